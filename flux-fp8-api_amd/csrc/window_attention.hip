// fluxmi -- shifted-window attention with a 2-D relative-position bias (the Swin block of SwinIR, modules/swinir.py; also Swin2SR's, HAT's
// and DAT's window core), gfx950.
//
// Swin computes  roll(-shift) -> window_partition -> softmax(q k^T * scale + bias [+ mask]) v -> window_reverse -> roll(+shift)  with four
// activation copies around a batched attention.  Here the partition, both rolls and the reverse are ADDRESS ARITHMETIC of one launch: token t
// of window (wy, wx) is rolled pixel (8 wy + t / 8, 8 wx + t % 8), i.e. source pixel ((i + shift) mod H, (j + shift) mod W), read there and
// written back there.  Arithmetic (the contract of include/fluxmi.h, restated by tests/swinir_ref.py):
//   s = fp32 MFMA sum of the bf16 products q . k over the head's 32 columns;   t = s * scale + bias_table[...][h] (+ -100 across mask regions)
//   m = max_j t (exact: the whole 64-key row is in registers),  p = exp(t - m) fp32,  l = sum p fp32,  O = sum bf16(p) v (MFMA, fp32)
//   out = bf16(O / l)                     one rounding of the output
//
// Shape.  One workgroup = one window of one image, ONE WAVE PER HEAD (up to WPB = 8 heads; more heads go to blockIdx.z), grid (windows, B,
// head groups).  A wave owns the head's whole 64 x 64 problem, so no partial result ever crosses waves.  Both products are "swapped"
// (vae_attention.hip): S^T = K Q^T and O^T = V^T P^T on the 32x32x16 bf16 MFMA, so an accumulator column is ONE query (lane & 31) and max,
// sum and 1 / l are per-lane scalars plus one exchange with the other lane half.
//   scores   four 32 x 32 tiles (key tile kt, query tile qt), two MFMAs each.  The K and Q operands are 16-byte runs along the head dimension,
//            loaded from the pixel rows straight into the operand registers: 8 loads per lane.
//   bias     the wave's 225-entry table column sits in LDS; in the MFMA output layout accumulator entry r of tile (kt, qt) is key row
//            4 kt + r / 4, key column 4 half + r % 4, so the table index is a per-lane base minus a compile-time offset.
//   mask     in that layout the key's region id is constant per (kt, lane half): rows split at the window's row 4 (= kt), columns at column 4
//            (= half).  The mask is therefore two comparisons per tile: last window row and qt != kt, last window column and (query column
//            >= 4) != half -- no id table, and H = 8 or W = 8 is the same rule.
//   P V      needs the KEY index along the MFMA's k dimension, where the score tiles hold it along rows.  The sum over keys does not care about
//            their order, so k-slot (half, j) of step (kt, g) is DEFINED as key 32 kt + 16 g + 8 (j / 4) + 4 half + j % 4: exactly the eight
//            p a lane already holds in accumulator entries 8 g .. 8 g + 7.  P never leaves its registers.  V is the one operand that goes
//            through LDS, once: 16-byte global loads of the pixel rows, stored transposed (V^T [d][key], pitch 68), read back as two 8-byte
//            runs of four keys per step.
//   store    O^T[d][query]: a lane holds four runs of four adjacent d of its query -> four 8-byte stores into the query's source pixel.
// A head narrower than 32 arrives zero-padded (q, k and v columns); zero v columns give O = 0 exactly, so the pad columns are stored as zero.
// LDS per workgroup: 8 x (32 x 68 x 2 + 225 x 4) = 42 KiB.  Nothing is atomic; blockIdx.y only offsets pointers.  Addresses are 64-bit.
#include "common.h"
#include "fluxmi_internal.h"

namespace {

constexpr int WS = FLUXMI_WINDOW;       // window edge
constexpr int NT = WS * WS;             // tokens per window
constexpr int HD = 32;                  // padded head width
constexpr int WPB = 8;                  // waves (= heads) per workgroup
constexpr int VT_LD = NT + 4;           // V^T row pitch in LDS (bf16): 136 bytes = 34 banks, so 32 rows' 8-byte reads meet no bank twice
constexpr int NB = (2 * WS - 1) * (2 * WS - 1);
static_assert(WS == 8 && NT == 64, "the lane roles below are written for 8 x 8 windows: two 32-token tiles of four window rows each");

struct WinAttnArgs {
  const u16* qkv; long long ld;   // [B][H][W] pixels: q | k | v, each heads * 32 columns
  const float* table;             // [225][heads]
  u16* out; long long ldo;        // [B][H][W] pixels, heads * 32 columns written
  int H, W, heads, shift;
  float scale;
};

__global__ void __launch_bounds__(WPB * 64) window_attention_kernel(const WinAttnArgs a) {
  __shared__ __align__(16) u16 s_vt[WPB][HD][VT_LD];
  __shared__ float s_tab[WPB][NB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, half = lane >> 5;
  const int h = blockIdx.z * WPB + wave;
  const bool live = h < a.heads;  // wave-uniform; idle waves of the last head group only meet the barrier
  const int nwx = a.W / WS;
  const int wy = blockIdx.x / nwx, wx = blockIdx.x - wy * nwx;
  const long long img = (long long)blockIdx.y * a.H * a.W;
  // source pixel of window token t (any t in 0..63), as an element offset of its pixel row
  auto pixel = [&](int t) -> long long {
    int sy = WS * wy + (t >> 3) + a.shift, sx = WS * wx + (t & 7) + a.shift;
    sy -= sy >= a.H ? a.H : 0;
    sx -= sx >= a.W ? a.W : 0;
    return img + (long long)sy * a.W + sx;
  };
  const int C = a.heads * HD;
  v8bf qf[2][2], kf[2][2];  // [tile][k-step]: token 32 tile + l31, columns 16 step + 8 half ..
  long long pix[2];
  if (live) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      pix[t] = pixel(32 * t + l31);
      const u16* p = a.qkv + pix[t] * a.ld + h * HD + half * 8;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        qf[t][s] = *(const v8bf*)(p + 16 * s);
        kf[t][s] = *(const v8bf*)(p + C + 16 * s);
      }
    }
    // V^T into LDS: chunk c = lane + 64 i is token c / 4, columns 8 (c % 4) ..
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = lane + 64 * i, tok = c >> 2, d0 = (c & 3) * 8;
      const uint4 v = *(const uint4*)(a.qkv + pixel(tok) * a.ld + 2 * C + h * HD + d0);
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s_vt[wave][d0 + 2 * j][tok] = (u16)(w[j] & 0xffffu);
        s_vt[wave][d0 + 2 * j + 1][tok] = (u16)(w[j] >> 16);
      }
    }
    for (int i = lane; i < NB; i += 64) s_tab[wave][i] = a.table[(long long)i * a.heads + h];
  }
  __syncthreads();
  if (!live) return;
  // ---- S^T tiles: acc[qt][kt][r] = key 32 kt + 8 (r / 4) + 4 half + r % 4 (window row 4 kt + r / 4, column 4 half + r % 4), query 32 qt + l31
  v16f acc[2][2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[qt][kt][r] = 0.f;
#pragma unroll
      for (int s = 0; s < 2; ++s) acc[qt][kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kt][s], qf[qt][s], acc[qt][kt], 0, 0, 0);
    }
  const bool last_row = a.shift > 0 && wy == a.H / WS - 1, last_col = a.shift > 0 && wx == nwx - 1;
  const int xa = l31 & 7;
  const bool col_cut = last_col && ((xa >= 4) != (half == 1));
  const float* tab = s_tab[wave];
  float lsum[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    // bias index (ya - yb + 7) * 15 + (xa - xb + 7), ya = 4 qt + l31 / 8, yb = 4 kt + r / 4, xb = 4 half + r % 4
    const int base = (4 * qt + (l31 >> 3) + 7) * 15 + xa + 7 - 4 * half;
    float m = -3.0e38f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      const float mask = (col_cut || (last_row && qt != kt)) ? -100.f : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float t = acc[qt][kt][r] * a.scale + tab[base - (4 * kt + (r >> 2)) * 15 - (r & 3)];
        t += mask;
        acc[qt][kt][r] = t;
        m = fmaxf(m, t);
      }
    }
    m = fmaxf(m, __shfl_xor(m, 32));
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = __expf(acc[qt][kt][r] - m);
        acc[qt][kt][r] = p;
        l += p;
      }
    l += __shfl_xor(l, 32);
    lsum[qt] = l;
  }
  // ---- O^T[d][query] = V^T P^T over four k-steps (kt, g); k-slot (half, j) = key 32 kt + 16 g + 8 (j / 4) + 4 half + j % 4
  v16f o[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[qt][r] = 0.f;
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const u16* vr = &s_vt[wave][l31][32 * kt + 16 * g + 4 * half];
      union { uint2 u[2]; v8bf v; } va;
      va.u[0] = *(const uint2*)vr;
      va.u[1] = *(const uint2*)(vr + 8);
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        union { unsigned u[4]; v8bf v; } pb;
#pragma unroll
        for (int j = 0; j < 4; ++j) pb.u[j] = pack_bf2(acc[qt][kt][8 * g + 2 * j], acc[qt][kt][8 * g + 2 * j + 1]);
        o[qt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va.v, pb.v, o[qt], 0, 0, 0);
      }
    }
  // ---- o[qt][r] = O^T[d = 8 (r / 4) + 4 half + r % 4][query 32 qt + l31]
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    u16* op = a.out + pix[qt] * a.ldo + h * HD + 4 * half;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = o[qt][4 * g + e] / lsum[qt];
      *(uint2*)(op + 8 * g) = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
    }
  }
}

// ---- LayerNorm over the first D channels of padded pixel rows (SwinIR's embed_dim 180 / 60 is no multiple of 8, which fluxmi_row_norm
// needs).  One wave per row, one 16-byte chunk per lane, the row held in registers between the passes: y = bf16((x - mean) * rstd * w + b)
// with mean and the centred variance over channels < D only.  w and b hold D8 = D rounded up to 8 entries, zero past D, so the columns
// [D, D8) are stored as exact zeros.
__global__ void __launch_bounds__(256) channel_norm_kernel(const u16* __restrict__ x, long long ldx, const u16* __restrict__ w,
                                                           const u16* __restrict__ b, u16* __restrict__ y, long long ldy, long long rows, int D,
                                                           float eps) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // wave-uniform, no barrier below
  const int c = lane * 8;
  const bool has = c < D;  // the chunk holds at least one real channel; it lies inside D8 <= ldx
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = 0.f;
  if (has) unpack8(*(const uint4*)(x + row * ldx + c), v);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) s += c + j < D ? v[j] : 0.f;
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) q += c + j < D ? (v[j] - mean) * (v[j] - mean) : 0.f;
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
  if (!has) return;
  float ww[8], bb[8], o[8];
  unpack8(*(const uint4*)(w + c), ww);
  unpack8(*(const uint4*)(b + c), bb);
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = c + j < D ? (v[j] - mean) * rstd * ww[j] + bb[j] : 0.f;
  *(uint4*)(y + row * ldy + c) = pack8(o);
}

}  // namespace

int fluxmi_k_channel_norm(const void* x, long long ldx, const void* weight, const void* bias, void* y, long long ldy, long long rows, int D,
                          float eps, hipStream_t s) {
  const int D8 = (D + 7) / 8 * 8;
  FLUXMI_REQUIRE(D >= 1 && D <= 512, "channel_norm: D=%d must be in 1..512 (one 16-byte chunk per lane of a wave)", D);
  FLUXMI_REQUIRE(rows >= 0 && (rows + 3) / 4 <= 2147483647LL, "channel_norm: rows=%lld exceed the launch grid", rows);
  FLUXMI_REQUIRE(x && weight && bias && y, "channel_norm: x, weight, bias and y must not be NULL");
  FLUXMI_REQUIRE(ldx % 8 == 0 && ldy % 8 == 0 && ldx >= D8 && ldy >= D8, "channel_norm: the row strides must be multiples of 8 and >= D rounded up to 8 = %d", D8);
  FLUXMI_REQUIRE(((uintptr_t)x | (uintptr_t)y | (uintptr_t)weight | (uintptr_t)bias) % 16 == 0, "channel_norm: x, y, weight and bias must be 16-byte aligned");
  if (rows == 0) return 0;
  hipLaunchKernelGGL(channel_norm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, (const u16*)x, ldx, (const u16*)weight,
                     (const u16*)bias, (u16*)y, ldy, rows, D, eps);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}

int fluxmi_k_window_attention(const void* qkv, long long ld, const float* bias_table, void* out, long long ldo, int B, int H, int W, int heads,
                              int shift, float scale, hipStream_t s) {
  FLUXMI_REQUIRE(H >= WS && W >= WS && H % WS == 0 && W % WS == 0, "window_attention: H=%d, W=%d must be positive multiples of the window %d", H, W, WS);
  FLUXMI_REQUIRE(shift == 0 || shift == WS / 2, "window_attention: shift=%d must be 0 or %d", shift, WS / 2);
  FLUXMI_REQUIRE(heads >= 1 && heads <= 16, "window_attention: heads=%d must be in 1..16", heads);
  const long long windows = (long long)(H / WS) * (W / WS);
  FLUXMI_REQUIRE(B >= 1 && B <= 65535 && windows <= 2147483647LL,
                 "window_attention: B=%d images / %lld windows exceed the launch grid (65535 / 2^31 - 1)", B, windows);
  FLUXMI_REQUIRE(qkv && bias_table && out, "window_attention: qkv, bias_table and out must not be NULL");
  const long long C = (long long)heads * HD;
  FLUXMI_REQUIRE(ld % 8 == 0 && ld >= 3 * C, "window_attention: the qkv pixel stride ld=%lld must be a multiple of 8 and >= 3 * heads * 32 = %lld", ld, 3 * C);
  FLUXMI_REQUIRE(ldo % 8 == 0 && ldo >= C, "window_attention: the out pixel stride ldo=%lld must be a multiple of 8 and >= heads * 32 = %lld", ldo, C);
  FLUXMI_REQUIRE(((uintptr_t)qkv | (uintptr_t)out) % 16 == 0 && (uintptr_t)bias_table % 4 == 0,
                 "window_attention: qkv and out must be 16-byte aligned (bias_table 4-byte)");
  const long long px = (long long)B * H * W;
  const uintptr_t q0 = (uintptr_t)qkv, q1 = q0 + (uintptr_t)(((px - 1) * ld + 3 * C) * 2);
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)(((px - 1) * ldo + C) * 2);
  FLUXMI_REQUIRE(o1 <= q0 || q1 <= o0, "window_attention: out must not overlap qkv (a window's queries are other windows' keys under a shift)");
  WinAttnArgs a;
  a.qkv = (const u16*)qkv; a.ld = ld; a.table = bias_table; a.out = (u16*)out; a.ldo = ldo;
  a.H = H; a.W = W; a.heads = heads; a.shift = shift; a.scale = scale;
  const dim3 grid((unsigned)windows, B, (heads + WPB - 1) / WPB);
  hipLaunchKernelGGL(window_attention_kernel, grid, dim3(64 * (heads < WPB ? heads : WPB)), 0, s, a);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}
