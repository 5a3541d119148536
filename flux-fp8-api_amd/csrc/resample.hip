// fluxmi -- the image resampler (gfx950): Pillow's 8-bit resize, byte for byte, on the device.  The arithmetic is stated in
// include/fluxmi.h (fluxmi_resample_*); the coefficient tables come from the host (resample_host.cpp) and everything here is integer.
//
// Images are uint8 [B][H][W][C], C in {1, 3}, with a row stride and an image stride in BYTES.  A resize is separable and a row is W * C
// bytes whose channels never mix, so the kernel works on BYTES: output byte e of a row belongs to pixel e / C, channel e % C.
//
// resample_kernel<MODE>   one workgroup (4 waves) = one tile of TB = 256 output bytes x TR = 16 output rows.
//   horizontal pass (FUSED, H_ONLY): the tile needs input rows [ylo, yhi) -- those its vertical taps touch; its own rows for H_ONLY -- cut to
//     the bytes [begin, xhi * C) its horizontal taps touch.  They pass through s_in (16 KiB) in chunks of as many whole rows as fit, loaded
//     as dwords by consecutive lanes.  Thread t owns output byte t of the tile for every row: it walks its coefficient row once per 8 staged
//     rows (one cached global load per tap, eight LDS byte reads and multiply-adds behind it) and writes the clipped bytes into s_mid, the
//     uint8 intermediate: row r of s_mid is row ylo + r of Pillow's temporary image, columns of this tile only.  It never goes to HBM.
//   vertical pass (FUSED, V_ONLY): wave v owns output rows v, v + 4, ... of the tile and lane l the dword l of each: a tap is ONE ds_read_b32
//     per lane at 64 consecutive dwords -- every bank once, no conflict -- and its coefficient is wave-uniform (row bounds through readfirstlane,
//     the table read through the constant address space), so it arrives by s_load_dword, not a per-lane load (profiles/resize.txt has the
//     assembly and the measurement against per-lane loads: the same kernel time).  Four int32 accumulators per dword, clipped, packed and stored as one dword per lane: 256
//     contiguous bytes per wave.  V_ONLY fills s_mid straight from the source, 128 rows at a time, keeping the accumulators across chunks,
//     so any reduction fits.
//   H_ONLY stores s_mid's rows as they are.
// Matrix instructions do not fit: the taps are 23-bit integers and the sum must be exact in int32; MFMA takes 8-bit integer operands.
#include "common.h"
#include "fluxmi_internal.h"

namespace {

typedef unsigned char u8;
constexpr int TB = FLUXMI_RESAMPLE_TILE_BYTES, TR = FLUXMI_RESAMPLE_TILE_ROWS;
constexpr int TDW = TB / 4;
constexpr int IN_DW = FLUXMI_RESAMPLE_LDS_IN_BYTES / 4;
constexpr int MID_ROWS = FLUXMI_RESAMPLE_LDS_MID_BYTES / TB;
constexpr int HALF = 1 << (FLUXMI_RESAMPLE_PRECISION_BITS - 1);
static_assert(TB == 256 && TDW == 64, "thread t owns byte t of a tile row in the horizontal pass, lane l dword l in the vertical pass");
static_assert(TR % 4 == 0 && TR <= MID_ROWS, "four waves share a tile's rows; H_ONLY keeps a whole tile in s_mid");
enum { FUSED = 0, H_ONLY = 1, V_ONLY = 2 };
// the coefficient tables are written before the launch and only read here: through the constant address space a wave-uniform address is a
// scalar load
typedef int __attribute__((address_space(4))) cint;

// four raw bytes at byte offset o (o % 4 == 0) of a row of row_bytes bytes; bytes outside the row read as 0 and are not touched
__device__ __forceinline__ unsigned load_row_dword(const u8* row, int o, int row_bytes, bool aligned) {
  if (aligned && o + 4 <= row_bytes) return *(const unsigned*)(row + o);
  unsigned v = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (o + e < row_bytes) v |= (unsigned)row[o + e] << (8 * e);
  return v;
}
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
__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> FLUXMI_RESAMPLE_PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}
// (xmin, n) of output index i, held inside [0, n_in) and ksize whatever the table says: no tap can leave the image
__device__ __forceinline__ void taps(const int* __restrict__ bounds, int i, int n_in, int ksize, int& lo, int& n) {
  lo = bounds[2 * i];
  n = bounds[2 * i + 1];
  lo = lo < 0 ? 0 : (lo > n_in ? n_in : lo);
  const int cap = ksize < n_in - lo ? ksize : n_in - lo;
  n = n < 0 ? 0 : (n > cap ? cap : n);
}

struct RsArgs {
  const u8* src; long long ld, bs;   // H x W source
  u8* dst; long long dld, dbs;       // h x w destination (h == H for H_ONLY, w == W for V_ONLY)
  const int* bx; const int* kx;
  const int* by; const int* ky;
  int ksx, ksy, H, W, C, h, w;
};

template <int MODE>
__global__ void __launch_bounds__(256) resample_kernel(const RsArgs a) {
  __shared__ unsigned s_in[MODE == V_ONLY ? 1 : IN_DW];
  __shared__ unsigned s_mid[MID_ROWS * TDW];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int e0 = blockIdx.x * TB, oy0 = blockIdx.y * TR;
  const int out_bytes = a.w * a.C;
  const int ne = out_bytes - e0 < TB ? out_bytes - e0 : TB;
  const int nr = a.h - oy0 < TR ? a.h - oy0 : TR;
  const u8* img = a.src + (long long)blockIdx.z * a.bs;
  u8* out = a.dst + (long long)blockIdx.z * a.dbs;

  int ylo = oy0, yhi = oy0 + nr;  // rows of the intermediate under this tile
  if (MODE != H_ONLY) {
    int n0, y1, n1;
    taps(a.by, oy0, a.H, a.ksy, ylo, n0);
    taps(a.by, oy0 + nr - 1, a.H, a.ksy, y1, n1);
    yhi = y1 + n1 > ylo ? y1 + n1 : ylo;
  }
  const int rows = yhi - ylo;
  if (MODE == FUSED && rows > MID_ROWS) return;  // the host plans the two-launch path for such a resize: never taken

  if (MODE != V_ONLY) {
    int xlo, xhi, n0, n1;
    taps(a.bx, e0 / a.C, a.W, a.ksx, xlo, n0);
    taps(a.bx, (e0 + ne - 1) / a.C, a.W, a.ksx, xhi, n1);
    xhi = xhi + n1 > xlo ? xhi + n1 : xlo;
    const int begin = (xlo * a.C) & ~3;
    int nd = (xhi * a.C - begin + 3) >> 2;
    nd = nd < 1 ? 1 : nd;
    if (nd > IN_DW) return;  // refused by the host: never taken
    const int px = (e0 + tid) / a.C, c = e0 + tid - px * a.C;
    const bool mine = tid < ne;
    int xmin = xlo, xn = 0;
    if (mine) {
      taps(a.bx, px, a.W, a.ksx, xmin, xn);
      xmin = xmin < xlo ? xlo : (xmin > xhi ? xhi : xmin);
      xn = xn > xhi - xmin ? xhi - xmin : xn;
    }
    const int* __restrict__ krow = a.kx + (long long)px * a.ksx;
    const u8* sb = (const u8*)s_in + (xmin * a.C + c - begin);
    u8* mb = (u8*)s_mid + tid;
    const int pitch = nd * 4, row_bytes = a.W * a.C;
    int ch = IN_DW / nd;
    ch = ch > rows ? rows : ch;
    for (int r0 = 0; r0 < rows; r0 += ch) {
      const int cr = rows - r0 < ch ? rows - r0 : ch;
      __syncthreads();  // the chunk before this one has been read
      for (int i = tid; i < cr * nd; i += 256) {
        const int r = i / nd, d = i - r * nd;
        const u8* row = img + (long long)(ylo + r0 + r) * a.ld;
        s_in[i] = load_row_dword(row, begin + 4 * d, row_bytes, aligned4(row));
      }
      __syncthreads();
      if (mine) {
        for (int r = 0; r < cr; r += 8) {
          int acc[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] = HALF;
          const u8* p = sb + r * pitch;
          for (int t = 0; t < xn; ++t) {
            const int k = krow[t];
#pragma unroll
            for (int j = 0; j < 8; ++j)
              if (r + j < cr) acc[j] += (int)p[j * pitch] * k;
            p += a.C;
          }
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (r + j < cr) mb[(r0 + r + j) * TB] = (u8)clip8(acc[j]);
        }
      }
    }
    __syncthreads();
  }

  if (MODE == H_ONLY) {
    for (int j = wv; j < nr; j += 4) {
      u8* row = out + (long long)(oy0 + j) * a.dld;
      store_row_dword(row, e0 + 4 * lane, out_bytes, aligned4(row), s_mid[j * TDW + lane]);
    }
    return;
  }

  // vertical pass: wave wv owns output rows oy0 + wv + 4 j, lane `lane` the dword `lane` of each
  int acc[TR / 4][4], ymin[TR / 4], yn[TR / 4];
#pragma unroll
  for (int j = 0; j < TR / 4; ++j) {
    ymin[j] = ylo;
    yn[j] = 0;
    if (wv + 4 * j < nr) {
      taps(a.by, oy0 + wv + 4 * j, a.H, a.ksy, ymin[j], yn[j]);
      ymin[j] = ymin[j] < ylo ? ylo : (ymin[j] > yhi ? yhi : ymin[j]);
      yn[j] = yn[j] > yhi - ymin[j] ? yhi - ymin[j] : yn[j];
    }
    ymin[j] = __builtin_amdgcn_readfirstlane(ymin[j]);  // the same in every lane: the tap loop and its coefficient address stay scalar
    yn[j] = __builtin_amdgcn_readfirstlane(yn[j]);
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[j][b] = HALF;
  }
  for (int c0 = ylo; c0 < yhi; c0 += MID_ROWS) {
    const int cr = yhi - c0 < MID_ROWS ? yhi - c0 : MID_ROWS;
    if (MODE == V_ONLY) {
      __syncthreads();
      for (int i = tid; i < cr * TDW; i += 256) {
        const int o = e0 + 4 * (i & 63);
        const u8* row = img + (long long)(c0 + (i >> 6)) * a.ld;
        s_mid[i] = o < out_bytes ? load_row_dword(row, o, out_bytes, aligned4(row)) : 0u;
      }
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < TR / 4; ++j) {
      const int t0 = c0 - ymin[j] > 0 ? c0 - ymin[j] : 0;
      const int t1 = c0 + cr - ymin[j] < yn[j] ? c0 + cr - ymin[j] : yn[j];
      const cint* krow = (const cint*)(uintptr_t)(a.ky + (long long)(oy0 + wv + 4 * j) * a.ksy);
      const int m = (ymin[j] - c0) * TDW + lane;  // row ymin + t of the intermediate is row ymin + t - c0 of s_mid
      for (int t = t0; t < t1; ++t) {
        const int k = krow[t];
        const unsigned v = s_mid[m + t * TDW];
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[j][b] += (int)((v >> (8 * b)) & 0xffu) * k;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < TR / 4; ++j) {
    if (wv + 4 * j >= nr) continue;
    unsigned v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) v |= (unsigned)clip8(acc[j][b]) << (8 * b);
    u8* row = out + (long long)(oy0 + wv + 4 * j) * a.dld;
    store_row_dword(row, e0 + 4 * lane, out_bytes, aligned4(row), v);
  }
}

template <int MODE>
void launch(const RsArgs& a, int B, hipStream_t s) {
  const dim3 grid((a.w * a.C + TB - 1) / TB, (a.h + TR - 1) / TR, B);
  hipLaunchKernelGGL(resample_kernel<MODE>, grid, dim3(256), 0, s, a);
}

int image_ok(const char* name, const void* p, long long ld, long long bs, int B, int H, int W, int C) {
  FLUXMI_REQUIRE(p, "resample_u8: %s must not be NULL", name);
  FLUXMI_REQUIRE(ld >= (long long)W * C, "resample_u8: %s row stride %lld is shorter than its W * C = %lld bytes", name, ld, (long long)W * C);
  FLUXMI_REQUIRE(B == 1 || bs >= (long long)H * ld, "resample_u8: %s image stride %lld is shorter than its H rows of %lld bytes", name, bs, ld);
  return 0;
}

}  // namespace

int fluxmi_k_resample_u8(const void* src, long long ld, long long bs, void* dst, long long dld, long long dbs, void* work, long long work_bytes,
                         int B, int H, int W, int C, int h, int w, int filter, const int* bounds_x, const int* kk_x, const int* bounds_y,
                         const int* kk_y, hipStream_t s) {
  FluxmiResamplePlan p;
  FLUXMI_TRY(fluxmi_resample_make_plan("resample_u8", B, H, W, C, h, w, filter, &p));
  FLUXMI_REQUIRE(H <= 65535 * TR && h <= 65535 * TR, "resample_u8: H=%d and h=%d must each fit the launch grid's limit of %d rows", H, h, 65535 * TR);
  FLUXMI_TRY(image_ok("src", src, ld, bs, B, H, W, C));
  FLUXMI_TRY(image_ok("dst", dst, dld, dbs, B, h, w, C));
  FLUXMI_REQUIRE(src != dst, "resample_u8: dst must not be src");
  FLUXMI_REQUIRE(!p.do_x || (bounds_x && kk_x), "resample_u8: the width changes (%d -> %d): bounds_x and kk_x must be device tables", W, w);
  FLUXMI_REQUIRE(!p.do_y || (bounds_y && kk_y), "resample_u8: the height changes (%d -> %d): bounds_y and kk_y must be device tables", H, h);
  if (p.work_bytes) {
    FLUXMI_REQUIRE(work && ((uintptr_t)work & 15) == 0, "resample_u8: this resize runs as two launches: work must be a 16-byte aligned device "
                   "buffer of fluxmi_resample_plan's size (%lld bytes)", p.work_bytes);
    FLUXMI_REQUIRE(work_bytes >= p.work_bytes, "resample_u8: work holds %lld bytes, fluxmi_resample_plan gives %lld", work_bytes, p.work_bytes);
  }
  RsArgs a;
  a.src = (const u8*)src; a.ld = ld; a.bs = bs; a.dst = (u8*)dst; a.dld = dld; a.dbs = dbs;
  a.bx = bounds_x; a.kx = kk_x; a.by = bounds_y; a.ky = kk_y; a.ksx = p.ax.ksize; a.ksy = p.ay.ksize;
  a.H = H; a.W = W; a.C = C; a.h = h; a.w = w;
  if (p.fused) {
    launch<FUSED>(a, B, s);
  } else if (p.do_x && p.do_y) {
    RsArgs hp = a, vp = a;
    hp.dst = (u8*)work; hp.dld = p.pitch; hp.dbs = p.pitch * H; hp.h = H;
    launch<H_ONLY>(hp, B, s);
    FLUXMI_LAUNCH_CHECK();
    vp.src = (const u8*)work; vp.ld = p.pitch; vp.bs = p.pitch * H; vp.W = w;
    launch<V_ONLY>(vp, B, s);
  } else if (p.do_x) {
    launch<H_ONLY>(a, B, s);
  } else if (p.do_y) {
    launch<V_ONLY>(a, B, s);
  } else {
    for (int b = 0; b < B; ++b)
      FLUXMI_CHECK_HIP(hipMemcpy2DAsync((u8*)dst + b * dbs, dld, (const u8*)src + b * bs, ld, (size_t)W * C, H, hipMemcpyDeviceToDevice, s));
    return 0;
  }
  FLUXMI_LAUNCH_CHECK();
  return 0;
}
