// fluxmi -- control-map preprocessors (gfx950): the classical ones that need no weights -- a Canny edge detector, PIL's luma, a separable
// Gaussian blur -- so that "photo -> control map -> resize -> VAE encode -> pack" stays on the device (FluxPipeline.preprocess_control).
// The arithmetic of every function here is stated in include/fluxmi.h; Canny and the luma are integer arithmetic and exact.
//
// Images are uint8 [B][H][W][C] with a row stride and an image stride in BYTES, so a caller may hand in a window of a larger buffer.  Every
// global access is 4 bytes wide where the row's address allows it (row base % 4 == 0 and the four bytes inside the row) and falls back to
// bytes elsewhere; nothing outside [0, W * C) of a row is ever read or written.
//
// canny_classify_kernel   one workgroup = one 32 x 32 pixel tile.  The tile's input with a 2-pixel halo (36 rows of 112 raw bytes, rows
//                         clamped at load, columns clamped at use: the replicated border) is staged in LDS once; the Sobel magnitude of the
//                         34 x 34 pixels of tile + 1 is computed once each into LDS (0 outside the image); then every thread classifies four
//                         adjacent pixels (non-maximum suppression + the two thresholds) and stores them as one dword.
// canny_hysteresis_kernel one round: the tile's state + a 1-pixel halo in LDS, weak pixels with a strong 8-neighbour promoted until the tile
//                         stops changing (a workgroup-uniform loop on a barrier-reduced flag, at most 32 * 32 trips), the promoted pixels of
//                         the tile's OWN interior stored, and *changed = 1 (a plain store) if there were any.  A neighbour's halo may be
//                         read before or after that neighbour's store of the same round: both are valid states of a monotone update whose
//                         fixed point is unique, so the closure is deterministic although the number of rounds need not be.  No workgroup
//                         waits on another; the host (fluxmi_k_canny_hysteresis) launches rounds until one changes nothing.
// rgb_to_gray_kernel      four pixels per thread: three dwords in, one out.
// blur_h_kernel / blur_v_kernel   the two passes of the Gaussian: uint8 -> fp32 rows (a 256-pixel row segment + radius staged in LDS as
//                         floats), then fp32 columns -> uint8 (a 32-row x 64-element tile + radius staged in LDS, 16-byte LDS reads, four
//                         elements per thread).  The intermediate stays fp32; the only rounding to uint8 is at the last store.
#include <math.h>

#include "common.h"
#include "fluxmi_internal.h"

namespace {

typedef unsigned char u8;
constexpr int T = FLUXMI_CANNY_TILE;
static_assert(T == 32, "the thread roles below give each of 256 threads four adjacent pixels of a 32 x 32 tile");

// four raw bytes at byte offset o (o % 4 == 0, may be negative) of a row of row_bytes bytes; bytes outside the row read as 0
__device__ __forceinline__ unsigned load_row_dword(const u8* row, int o, int row_bytes, bool aligned) {
  if (aligned && o >= 0 && o + 4 <= row_bytes) return *(const unsigned*)(row + o);
  unsigned v = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (o + e >= 0 && o + e < row_bytes) v |= (unsigned)row[o + e] << (8 * e);
  return v;
}
// the reverse: bytes [o, o + 4) of a row, those inside [0, row_bytes)
__device__ __forceinline__ void store_row_dword(u8* row, int o, int row_bytes, bool aligned, unsigned v) {
  if (aligned && o + 4 <= row_bytes) {
    *(unsigned*)(row + o) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (o + e < row_bytes) row[o + e] = (u8)(v >> (8 * e));
  }
}
__device__ __forceinline__ bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

// ---- Canny: Sobel magnitude, non-maximum suppression, thresholds ---------------------------------------------------------------------
struct CannyArgs {
  const u8* rgb; long long ld, bs;
  u8* st; long long sld, sbs;
  int H, W, lo, hi, l2;
};

constexpr int IN_ROWS = T + 4;                // tile + 2-pixel halo
constexpr int IN_DW = (IN_ROWS * 3 + 4) / 4;  // 108 bytes of pixels behind a 2-byte lead that makes the first byte a dword boundary: 28
constexpr int MT = T + 2;                     // magnitudes: tile + 1

__global__ void __launch_bounds__(256) canny_classify_kernel(const CannyArgs a) {
  __shared__ unsigned s_in[IN_ROWS][IN_DW];
  __shared__ int s_m[MT][MT];
  __shared__ int s_d[MT][MT];  // dx in the low half, dy in the high half (|dx|, |dy| <= 1020)
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * T, y0 = blockIdx.y * T;
  const u8* img = a.rgb + (long long)blockIdx.z * a.bs;
  const int row_bytes = a.W * 3;
  const int byte0 = x0 * 3 - 8;  // the row byte that LDS byte 0 holds: pixel x0 - 2 is at LDS byte 2

  for (int i = tid; i < IN_ROWS * IN_DW; i += 256) {
    const int r = i / IN_DW, d = i - r * IN_DW;
    int gy = y0 - 2 + r;
    gy = gy < 0 ? 0 : (gy > a.H - 1 ? a.H - 1 : gy);
    const u8* row = img + (long long)gy * a.ld;
    s_in[r][d] = load_row_dword(row, byte0 + 4 * d, row_bytes, aligned4(row));
  }
  __syncthreads();

  for (int i = tid; i < MT * MT; i += 256) {
    const int my = i / MT, mx = i - my * MT;
    const int gy = y0 - 1 + my, gx = x0 - 1 + mx;
    int bm = 0, bdx = 0, bdy = 0;
    if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
      const int xl = (gx > 0 ? gx - 1 : 0) * 3 - byte0, xc = gx * 3 - byte0, xr = (gx < a.W - 1 ? gx + 1 : gx) * 3 - byte0;
      const u8* r0 = (const u8*)s_in[my];  // image rows gy - 1, gy, gy + 1, clamped when they were loaded
      const u8* r1 = (const u8*)s_in[my + 1];
      const u8* r2 = (const u8*)s_in[my + 2];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int p00 = r0[xl + c], p01 = r0[xc + c], p02 = r0[xr + c];
        const int p10 = r1[xl + c], p12 = r1[xr + c];
        const int p20 = r2[xl + c], p21 = r2[xc + c], p22 = r2[xr + c];
        const int dx = (p02 + 2 * p12 + p22) - (p00 + 2 * p10 + p20);
        const int dy = (p20 + 2 * p21 + p22) - (p00 + 2 * p01 + p02);
        const int m = a.l2 ? dx * dx + dy * dy : abs(dx) + abs(dy);
        if (c == 0 || m > bm) { bm = m; bdx = dx; bdy = dy; }
      }
    }
    s_m[my][mx] = bm;
    s_d[my][mx] = (int)((unsigned)(bdx & 0xffff) | ((unsigned)bdy << 16));
  }
  __syncthreads();

  const int ty = tid >> 3, tx = (tid & 7) * 4;
  const int gy = y0 + ty;
  if (gy >= a.H || x0 + tx >= a.W) return;
  unsigned out = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int my = ty + 1, mx = tx + e + 1;
    const int m = s_m[my][mx];
    unsigned v = 0;
    if (m > a.lo) {
      const int d = s_d[my][mx];
      const int dx = (int)(short)(d & 0xffff), dy = d >> 16;
      const int x = abs(dx), y = abs(dy) << 15;
      const int t22 = x * 13573, t67 = t22 + (x << 16);
      bool keep;
      if (y < t22) {
        keep = m > s_m[my][mx - 1] && m >= s_m[my][mx + 1];
      } else if (y > t67) {
        keep = m > s_m[my - 1][mx] && m >= s_m[my + 1][mx];
      } else {
        const int s = (dx ^ dy) < 0 ? -1 : 1;
        keep = m > s_m[my - 1][mx - s] && m > s_m[my + 1][mx + s];
      }
      if (keep) v = m > a.hi ? 2u : 1u;
    }
    out |= v << (8 * e);
  }
  u8* row = a.st + (long long)blockIdx.z * a.sbs + (long long)gy * a.sld;
  store_row_dword(row, x0 + tx, a.W, aligned4(row), out);
}

// ---- Canny: one hysteresis round ------------------------------------------------------------------------------------------------------
constexpr int HP = T + 8;  // LDS row pitch in bytes: interior column x at byte 4 + x, the halo columns at bytes 3 and 4 + T

__global__ void __launch_bounds__(256) canny_hysteresis_kernel(u8* st, long long sld, long long sbs, int H, int W, int* changed) {
  __shared__ unsigned s_w[(T + 2) * HP / 4];
  u8* s = (u8*)s_w;
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * T, y0 = blockIdx.y * T;
  u8* img = st + (long long)blockIdx.z * sbs;
  const int ty = tid >> 3, tx = (tid & 7) * 4;
  const int gy = y0 + ty;
  u8* row = img + (long long)gy * sld;
  const bool al = aligned4(row);
  unsigned cur = 0;
  if (gy < H && x0 + tx < W) cur = load_row_dword(row, x0 + tx, W, al);
  s_w[((ty + 1) * HP + 4 + tx) >> 2] = cur;
  if (tid < 4 * T + 4) {  // the halo ring: top and bottom rows (T + 2 each), left and right columns (T each); 0 outside the image
    int hy, hx;
    if (tid < T + 2) { hy = -1; hx = tid - 1; }
    else if (tid < 2 * T + 4) { hy = T; hx = tid - (T + 2) - 1; }
    else if (tid < 3 * T + 4) { hy = tid - (2 * T + 4); hx = -1; }
    else { hy = tid - (3 * T + 4); hx = T; }
    const int y = y0 + hy, x = x0 + hx;
    u8 v = 0;
    if (y >= 0 && y < H && x >= 0 && x < W) v = img[(long long)y * sld + x];
    s[(hy + 1) * HP + 4 + hx] = v;
  }
  __syncthreads();

  bool mine = false;
  const int base = ((ty + 1) * HP + 4 + tx) >> 2;  // this thread's dword; the rows above / below are HP / 4 dwords away
  for (int it = 0; it < T * T; ++it) {
    bool ch = false;
    if (cur & 0x01010101u) {  // a weak pixel among the four
      // six bytes per row: columns tx - 1 .. tx + 4; only bit 1 (set in "strong" = 2 alone) is looked at
      unsigned long long win[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int q = base + (r - 1) * (HP / 4);
        const unsigned lft = s_w[q - 1], mid = r == 1 ? cur : s_w[q], rgt = s_w[q + 1];
        win[r] = (unsigned long long)(lft >> 24) | ((unsigned long long)mid << 8) | ((unsigned long long)(rgt & 0xffu) << 40);
      }
      const unsigned long long ud = (win[0] | win[2]) & 0x020202020202ull;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (((cur >> (8 * e)) & 0xffu) != 1u) continue;
        const unsigned long long own = (win[1] | ((unsigned long long)cur << 8)) & 0x020202020202ull;
        if (((ud >> (8 * e)) & 0x020202ull) | ((own >> (8 * e)) & 0x020002ull)) {
          cur = (cur & ~(0xffu << (8 * e))) | (2u << (8 * e));
          ch = true;
        }
      }
      if (ch) s_w[base] = cur;  // only this thread writes this dword
    }
    mine |= ch;
    if (!__syncthreads_or(ch)) break;
  }
  if (mine) store_row_dword(row, x0 + tx, W, al, cur);  // never taken outside the image: nothing there is weak
  if (__syncthreads_or(mine) && tid == 0) *changed = 1;
}

// edges = 255 where state == 2, else 0; four pixels per thread
__global__ void __launch_bounds__(256) canny_edges_kernel(const u8* st, long long sld, long long sbs, u8* out, long long old, long long obs,
                                                          int H, int W) {
  const int x = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y;
  if (x >= W) return;
  const u8* srow = st + (long long)blockIdx.z * sbs + (long long)y * sld;
  u8* orow = out + (long long)blockIdx.z * obs + (long long)y * old;
  const unsigned v = load_row_dword(srow, x, W, aligned4(srow));
  store_row_dword(orow, x, W, aligned4(orow), ((v >> 1) & 0x01010101u) * 255u);
}

// ---- luma ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) rgb_to_gray_kernel(const u8* rgb, long long ld, long long bs, u8* gray, long long gld, long long gbs,
                                                          int H, int W) {
  const int x = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y;
  if (x >= W) return;
  const u8* row = rgb + (long long)blockIdx.z * bs + (long long)y * ld;
  u8* grow = gray + (long long)blockIdx.z * gbs + (long long)y * gld;
  const bool al = aligned4(row);
  unsigned w[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) w[k] = load_row_dword(row, x * 3 + 4 * k, W * 3, al);
  unsigned out = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    unsigned ch[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int byte = 3 * e + c;
      ch[c] = (w[byte >> 2] >> (8 * (byte & 3))) & 0xffu;
    }
    out |= ((19595u * ch[0] + 38470u * ch[1] + 7471u * ch[2] + 32768u) >> 16) << (8 * e);
  }
  store_row_dword(grow, x, W, aligned4(grow), out);
}

// ---- Gaussian blur ---------------------------------------------------------------------------------------------------------------------
struct BlurTaps {
  float w[FLUXMI_BLUR_MAX_RADIUS + 1];  // w[|i|], normalised over -r .. r
  int r;
};
constexpr int BH_TW = 256;                       // horizontal pass: pixels of one row per workgroup
constexpr int BV_TH = 32, BV_TE = 64;            // vertical pass: rows x elements per workgroup
constexpr int RMAX = FLUXMI_BLUR_MAX_RADIUS;

template <int C>
__global__ void __launch_bounds__(256) blur_h_kernel(const u8* src, long long ld, long long bs, float* tmp, long long P, int H, int W,
                                                     const BlurTaps tp) {
  __shared__ unsigned s_raw[((BH_TW + 2 * RMAX) * C + 3) / 4 + 2];
  __shared__ float s_f[(BH_TW + 2 * RMAX) * C];
  const int tid = threadIdx.x, r = tp.r;
  const int x0 = blockIdx.x * BH_TW, y = blockIdx.y;
  const u8* row = src + (long long)blockIdx.z * bs + (long long)y * ld;
  const int lo_px = x0 - r > 0 ? x0 - r : 0, hi_px = x0 + BH_TW + r < W ? x0 + BH_TW + r : W;
  const int begin = (lo_px * C) & ~3, nd = (hi_px * C - begin + 3) >> 2;
  const bool al = aligned4(row);
  for (int d = tid; d < nd; d += 256) s_raw[d] = load_row_dword(row, begin + 4 * d, W * C, al);
  __syncthreads();
  const int n = (BH_TW + 2 * r) * C;
  for (int j = tid; j < n; j += 256) {
    const int px = j / C, c = j - px * C;
    int gx = x0 - r + px;
    gx = gx < 0 ? 0 : (gx > W - 1 ? W - 1 : gx);
    s_f[j] = (float)((const u8*)s_raw)[gx * C + c - begin];
  }
  __syncthreads();
  float* trow = tmp + ((long long)blockIdx.z * H + y) * P + (long long)x0 * C;
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const int e = tid + 256 * k;
    if (x0 + e / C >= W) continue;
    float acc = 0.f;
    for (int i = 0; i <= 2 * r; ++i) acc = __builtin_fmaf(tp.w[i < r ? r - i : i - r], s_f[e + i * C], acc);
    trow[e] = acc;
  }
}

__global__ void __launch_bounds__(256) blur_v_kernel(const float* tmp, long long P, u8* dst, long long ld, long long bs, int H, int NE,
                                                     const BlurTaps tp) {
  __shared__ __align__(16) float s[(BV_TH + 2 * RMAX) * BV_TE];
  const int tid = threadIdx.x, r = tp.r;
  const int e0 = blockIdx.x * BV_TE, y0 = blockIdx.y * BV_TH;
  const float* tb = tmp + (long long)blockIdx.z * H * P;
  const int rows = BV_TH + 2 * r;
  for (int i = tid; i < rows * (BV_TE / 4); i += 256) {
    const int rr = i / (BV_TE / 4), q = i - rr * (BV_TE / 4);
    int gy = y0 - r + rr;
    gy = gy < 0 ? 0 : (gy > H - 1 ? H - 1 : gy);
    const int e = e0 + 4 * q;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < P) v = *(const float4*)(tb + (long long)gy * P + e);  // P % 4 == 0: the four floats are inside the row
    *(float4*)&s[rr * BV_TE + 4 * q] = v;
  }
  __syncthreads();
  const int tx = tid & 15, ty = tid >> 4;
  const int e = e0 + 4 * tx;
  if (e >= NE) return;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int oy = 2 * ty + j, gy = y0 + oy;
    if (gy >= H) continue;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i <= 2 * r; ++i) {
      const float w = tp.w[i < r ? r - i : i - r];
      const float4 v = *(const float4*)&s[(oy + i) * BV_TE + 4 * tx];
      acc[0] = __builtin_fmaf(w, v.x, acc[0]); acc[1] = __builtin_fmaf(w, v.y, acc[1]);
      acc[2] = __builtin_fmaf(w, v.z, acc[2]); acc[3] = __builtin_fmaf(w, v.w, acc[3]);
    }
    unsigned out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float q = rintf(acc[k]);
      out |= (unsigned)(q > 0.f ? (q < 255.f ? q : 255.f) : 0.f) << (8 * k);
    }
    u8* row = dst + (long long)blockIdx.z * bs + (long long)gy * ld;
    store_row_dword(row, e, NE, aligned4(row), out);
  }
}

// a [B][H][W][C] uint8 image whose rows hold W * C bytes: strides long enough that rows and images do not overlap, and a launch grid that fits
int image_ok(const char* who, const char* name, const void* p, long long ld, long long bs, int B, int H, int W, int C) {
  FLUXMI_REQUIRE(p, "%s: %s must not be NULL", who, name);
  FLUXMI_REQUIRE(ld >= (long long)W * C, "%s: %s row stride %lld is shorter than its W * C = %lld bytes", who, name, ld, (long long)W * C);
  FLUXMI_REQUIRE(B == 1 || bs >= (long long)H * ld, "%s: %s image stride %lld is shorter than its H rows of %lld bytes", who, name, bs, ld);
  return 0;
}
int shape_ok(const char* who, int B, int H, int W) {
  FLUXMI_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: B=%d, H=%d, W=%d must be >= 1", who, B, H, W);
  FLUXMI_REQUIRE(B <= 65535 && H <= 65535 && W <= (1 << 24), "%s: B=%d and H=%d must each fit the launch grid's limit of 65535, W=%d 2^24", who,
                 B, H, W);
  return 0;
}

}  // namespace

int fluxmi_k_canny_classify(const void* rgb, long long ld, long long bs, void* state, long long sld, long long sbs, int B, int H, int W,
                            int low, int high, int l2, hipStream_t s) {
  FLUXMI_TRY(shape_ok("canny_classify", B, H, W));
  FLUXMI_TRY(image_ok("canny_classify", "rgb", rgb, ld, bs, B, H, W, 3));
  FLUXMI_TRY(image_ok("canny_classify", "state", state, sld, sbs, B, H, W, 1));
  FLUXMI_REQUIRE(low >= 0 && high >= 0, "canny_classify: thresholds low=%d, high=%d must be >= 0", low, high);
  FLUXMI_REQUIRE(l2 == 0 || l2 == 1, "canny_classify: l2=%d must be 0 or 1", l2);
  long long lo = low < high ? low : high, hi = low < high ? high : low;
  if (l2) {  // compared with dx^2 + dy^2 <= 2 * 1020^2: a square beyond int saturates (no magnitude exceeds it either way)
    lo = lo * lo < 0x7fffffffLL ? lo * lo : 0x7fffffffLL;
    hi = hi * hi < 0x7fffffffLL ? hi * hi : 0x7fffffffLL;
  }
  CannyArgs a;
  a.rgb = (const u8*)rgb; a.ld = ld; a.bs = bs; a.st = (u8*)state; a.sld = sld; a.sbs = sbs;
  a.H = H; a.W = W; a.lo = (int)lo; a.hi = (int)hi; a.l2 = l2;
  hipLaunchKernelGGL(canny_classify_kernel, dim3((W + T - 1) / T, (H + T - 1) / T, B), dim3(256), 0, s, a);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}

int fluxmi_k_canny_hysteresis_round(void* state, long long sld, long long sbs, int B, int H, int W, int* changed_flag, hipStream_t s) {
  FLUXMI_TRY(shape_ok("canny_hysteresis_round", B, H, W));
  FLUXMI_TRY(image_ok("canny_hysteresis_round", "state", state, sld, sbs, B, H, W, 1));
  FLUXMI_REQUIRE(changed_flag && ((uintptr_t)changed_flag & 3) == 0, "canny_hysteresis_round: changed_flag must be a 4-byte aligned device int");
  hipLaunchKernelGGL(canny_hysteresis_kernel, dim3((W + T - 1) / T, (H + T - 1) / T, B), dim3(256), 0, s, (u8*)state, sld, sbs, H, W,
                     changed_flag);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}

int fluxmi_k_canny_hysteresis(void* state, long long sld, long long sbs, void* edges, long long eld, long long ebs, int* flags, int B, int H,
                              int W, int* rounds_out, hipStream_t s) {
  constexpr int G = FLUXMI_CANNY_ROUND_GROUP;
  FLUXMI_TRY(shape_ok("canny_hysteresis", B, H, W));
  FLUXMI_TRY(image_ok("canny_hysteresis", "state", state, sld, sbs, B, H, W, 1));
  FLUXMI_TRY(image_ok("canny_hysteresis", "edges", edges, eld, ebs, B, H, W, 1));
  FLUXMI_REQUIRE(flags && ((uintptr_t)flags & 3) == 0, "canny_hysteresis: flags must be %d 4-byte aligned device ints", G);
  // every round but the last promotes at least one pixel of some image: H * W + 1 rounds always suffice
  const long long max_rounds = (long long)H * W + 1;
  long long rounds = 0;
  for (bool done = false; !done;) {
    FLUXMI_REQUIRE(rounds < max_rounds, "canny_hysteresis: no fixed point after %lld rounds of a %d x %d image (the state map holds values "
                   "other than 0 / 1 / 2?)", rounds, H, W);
    const int n = max_rounds - rounds < G ? (int)(max_rounds - rounds) : G;
    int host[G];
    FLUXMI_CHECK_HIP(hipMemsetAsync(flags, 0, sizeof(int) * G, s));
    for (int k = 0; k < n; ++k) FLUXMI_TRY(fluxmi_k_canny_hysteresis_round(state, sld, sbs, B, H, W, flags + k, s));
    FLUXMI_CHECK_HIP(hipMemcpyAsync(host, flags, sizeof(int) * n, hipMemcpyDeviceToHost, s));
    FLUXMI_CHECK_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < n && !done; ++k) {  // the rounds behind the first unchanged one found a fixed point and did nothing
      ++rounds;
      done = host[k] == 0;
    }
  }
  hipLaunchKernelGGL(canny_edges_kernel, dim3((W + 1023) / 1024, H, B), dim3(256), 0, s, (const u8*)state, sld, sbs, (u8*)edges, eld, ebs, H, W);
  FLUXMI_LAUNCH_CHECK();
  if (rounds_out) *rounds_out = (int)(rounds < 0x7fffffffLL ? rounds : 0x7fffffffLL);
  return 0;
}

int fluxmi_k_canny(const void* rgb, long long ld, long long bs, void* edges, long long eld, long long ebs, void* work, long long work_bytes,
                   int B, int H, int W, int low, int high, int l2, int* rounds_out, hipStream_t s) {
  FLUXMI_TRY(shape_ok("canny", B, H, W));
  FLUXMI_REQUIRE(work && ((uintptr_t)work & 15) == 0, "canny: work must be a 16-byte aligned device buffer");
  const long long sld = ((long long)W + 3) & ~3LL, sbs = sld * H;
  FLUXMI_REQUIRE(work_bytes >= FLUXMI_CANNY_WORK_BYTES(B, H, W), "canny: work holds %lld bytes, FLUXMI_CANNY_WORK_BYTES(%d, %d, %d) = %lld",
                 work_bytes, B, H, W, (long long)FLUXMI_CANNY_WORK_BYTES(B, H, W));
  FLUXMI_TRY(image_ok("canny", "edges", edges, eld, ebs, B, H, W, 1));
  FLUXMI_TRY(fluxmi_k_canny_classify(rgb, ld, bs, work, sld, sbs, B, H, W, low, high, l2, s));
  return fluxmi_k_canny_hysteresis(work, sld, sbs, edges, eld, ebs, (int*)((u8*)work + sbs * B), B, H, W, rounds_out, s);
}

int fluxmi_k_rgb_to_gray(const void* rgb, long long ld, long long bs, void* gray, long long gld, long long gbs, int B, int H, int W,
                         hipStream_t s) {
  FLUXMI_TRY(shape_ok("rgb_to_gray", B, H, W));
  FLUXMI_TRY(image_ok("rgb_to_gray", "rgb", rgb, ld, bs, B, H, W, 3));
  FLUXMI_TRY(image_ok("rgb_to_gray", "gray", gray, gld, gbs, B, H, W, 1));
  hipLaunchKernelGGL(rgb_to_gray_kernel, dim3((W + 1023) / 1024, H, B), dim3(256), 0, s, (const u8*)rgb, ld, bs, (u8*)gray, gld, gbs, H, W);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}

int fluxmi_k_gaussian_blur(const void* src, long long ld, long long bs, void* dst, long long dld, long long dbs, void* work, long long work_bytes,
                           int B, int H, int W, int C, float sigma, hipStream_t s) {
  FLUXMI_TRY(shape_ok("gaussian_blur", B, H, W));
  FLUXMI_REQUIRE(C == 1 || C == 3, "gaussian_blur: C=%d must be 1 or 3", C);
  FLUXMI_TRY(image_ok("gaussian_blur", "src", src, ld, bs, B, H, W, C));
  FLUXMI_TRY(image_ok("gaussian_blur", "dst", dst, dld, dbs, B, H, W, C));
  FLUXMI_REQUIRE(src != dst, "gaussian_blur: dst must not be src");
  FLUXMI_REQUIRE(sigma > 0.f && sigma <= (float)FLUXMI_BLUR_MAX_RADIUS, "gaussian_blur: sigma=%g must be a positive number", (double)sigma);
  const int r = (int)ceil(3.0 * (double)sigma);
  FLUXMI_REQUIRE(r >= 1 && r <= FLUXMI_BLUR_MAX_RADIUS, "gaussian_blur: sigma=%g gives the radius ceil(3 sigma) = %d, outside 1..%d",
                 (double)sigma, r, FLUXMI_BLUR_MAX_RADIUS);
  FLUXMI_REQUIRE(work && ((uintptr_t)work & 15) == 0, "gaussian_blur: work must be a 16-byte aligned device buffer");
  FLUXMI_REQUIRE(work_bytes >= FLUXMI_BLUR_WORK_BYTES(B, H, W, C), "gaussian_blur: work holds %lld bytes, FLUXMI_BLUR_WORK_BYTES(%d, %d, %d, %d) "
                 "= %lld", work_bytes, B, H, W, C, (long long)FLUXMI_BLUR_WORK_BYTES(B, H, W, C));
  BlurTaps tp;
  double w[FLUXMI_BLUR_MAX_RADIUS + 1], sum = 0.0;
  const double sg = (double)sigma;
  for (int i = 0; i <= r; ++i) {
    w[i] = exp(-(double)i * i / (2.0 * sg * sg));
    sum += i ? 2.0 * w[i] : w[i];
  }
  for (int i = 0; i <= FLUXMI_BLUR_MAX_RADIUS; ++i) tp.w[i] = i <= r ? (float)(w[i] / sum) : 0.f;
  tp.r = r;
  const long long P = ((long long)W * C + 3) & ~3LL;
  const int NE = W * C;
  const dim3 gh((W + BH_TW - 1) / BH_TW, H, B);
  if (C == 1) hipLaunchKernelGGL(blur_h_kernel<1>, gh, dim3(256), 0, s, (const u8*)src, ld, bs, (float*)work, P, H, W, tp);
  else hipLaunchKernelGGL(blur_h_kernel<3>, gh, dim3(256), 0, s, (const u8*)src, ld, bs, (float*)work, P, H, W, tp);
  FLUXMI_LAUNCH_CHECK();
  hipLaunchKernelGGL(blur_v_kernel, dim3((NE + BV_TE - 1) / BV_TE, (H + BV_TH - 1) / BV_TH, B), dim3(256), 0, s, (const float*)work, P, (u8*)dst,
                     dld, dbs, H, NE, tp);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}
