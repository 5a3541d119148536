// fluxmi -- IP-Adapter: the decoupled image cross-attention of a double block (XLabs IPDoubleStreamBlockProcessor, restated; DESIGN.md
// section 7), one launch per double block:   x_img += ip_scale * softmax(qn . k_ip^T / sqrt(128)) . v_ip   over Nk <= 64 image tokens.
//
// Rounding points (include/fluxmi.h, fluxmi_ip_attention):
//   qn    the raw image q of the block's qkv GEMM, QK-RMSNorm'ed by the helper attention's raw-Q mode uses (attention_common.h, qknorm_rinv /
//         qknorm_apply: fp32 rms, eps 1e-6, bf16((x / rms) * w)), before RoPE: the same query bits as attention's
//   t_j   = (qn . k_j) * (128^-1/2 * log2 e) in fp32: each lane of a pair chains its 64 products by fma in (c, j) order, the two halves are added
//   p_j   = exp2(t_j - max t), acc = fma(p_j, v_j, acc), l = sum_j p_j in fp32, j ascending;  o = bf16(acc * (1 / l)): ONE rounding
//   fused x = bf16(x + bf16(o * s)), s the sample's fp32 device scalar: the arithmetic of add_scaled_kernel on the bf16 o, no contraction
//
// Shape of the work: the kernel is bound by bytes -- per (row, head) 256 B of q and, fused, 256 B of x read and written, against
// 2 * Nk * 256 flop -- so it stays on the VALU with 16-byte accesses and no MFMA.  A workgroup = 4 waves = 128 rows of ONE head; the head's
// Nk keys and values (Nk * 512 B) are staged in LDS once per workgroup and read as wave-wide broadcasts.  Lanes l and l + 32 of a wave share
// a row like the two lane halves of attention's Q fragments: lane half `hi` owns elements d = c*16 + hi*8 + [0, 8), c < 8.  The Nk scores of
// a row are parked in LDS between the two passes (Nk is a run-time value: a register array would go to scratch), so q (64 VGPRs) is dead
// before the 64 accumulators are live.
#include "attention_common.h"

namespace {

constexpr int IP_ROWS = 128;  // rows per workgroup: 4 waves x 32 lane pairs
constexpr int IP_MAX_NK = 64;

template <bool FUSED>
__global__ void __launch_bounds__(256) ip_attention_kernel(const u16* __restrict__ qkv, long long ld_qkv, long long qkv_bstride,
                                                           const u16* __restrict__ qn_scale, const u16* __restrict__ k_ip,
                                                           const u16* __restrict__ v_ip, long long kv_bstride, u16* out, long long ld_o,
                                                           long long o_bstride, const float* __restrict__ scale, long long scale_bstride,
                                                           int rows, int heads, int Nk) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ip_lds[];
  u16* ks = (u16*)ip_lds;                              // [Nk][128] bf16
  u16* vs = ks + Nk * 128;                             // [Nk][128] bf16
  float* ts = (float*)(ip_lds + (size_t)Nk * 512);     // [Nk][IP_ROWS] scores
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
  const int h = blockIdx.y, b = blockIdx.z;
  const int item = wave * 32 + l31;
  const int row_raw = blockIdx.x * IP_ROWS + item;
  const bool valid = row_raw < rows;
  const int row = valid ? row_raw : rows - 1;          // lanes past the end redo the last row (no divergence around the lane swaps), store nothing

  // the head's keys and values: rows [0, Nk) only, 16 B per thread and trip
  {
    const u16* kb = k_ip + (long long)b * kv_bstride + h * 128;
    const u16* vb = v_ip + (long long)b * kv_bstride + h * 128;
    const long long ldk = (long long)heads * 128;
    for (int i = tid; i < Nk * 16; i += 256) {
      const int j = i >> 4, c = (i & 15) * 8;
      *(uint4*)(ks + j * 128 + c) = *(const uint4*)(kb + j * ldk + c);
      *(uint4*)(vs + j * 128 + c) = *(const uint4*)(vb + j * ldk + c);
    }
  }

  // qn: the attention kernel's own QKNorm of the raw row (before RoPE)
  float x[8][8];
  {
    const u16* qp = qkv + (long long)b * qkv_bstride + (long long)row * ld_qkv + (long long)h * 128 + hi * 8;
    const u16* wn = qn_scale + hi * 8;
    uint4 raw[8], rw[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      raw[c] = *(const uint4*)(qp + c * 16);
      rw[c] = *(const uint4*)(wn + c * 16);
    }
    const float rinv = qknorm_rinv(raw, x);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float w[8];
      unpack8(rw[c], w);
      qknorm_apply(x[c], rinv, w);
    }
  }
  __syncthreads();

  // pass 1: scores in the exp2 domain, their maximum
  const float fold = 0.088388347648318440550f * 1.4426950408889634074f;  // 128^-1/2 * log2 e
  float m = -INFINITY;
  for (int j = 0; j < Nk; ++j) {
    const u16* kr = ks + j * 128 + hi * 8;
    float d = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float kf[8];
      unpack8(*(const uint4*)(kr + c * 16), kf);
#pragma unroll
      for (int e = 0; e < 8; ++e) d = fmaf(x[c][e], kf[e], d);
    }
    {  // the other half of the row's products sits in lane ^ 32 (the sum of the two halves is the same value in both lanes)
      const unsigned u = __float_as_uint(d);
      const auto sw2 = __builtin_amdgcn_permlane32_swap(u, u, false, false);
      d = __uint_as_float(sw2[0]) + __uint_as_float(sw2[1]);
    }
    const float t = d * fold;
    m = fmaxf(m, t);
    ts[j * IP_ROWS + item] = t;  // both lanes of the pair store the same value; each reads back what it stored
  }

  // pass 2: p = exp2(t - m), the row sum, p . v
  float acc[8][8];
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[c][e] = 0.f;
  float l = 0.f;
  for (int j = 0; j < Nk; ++j) {
    const float p = exp2f(ts[j * IP_ROWS + item] - m);
    l += p;
    const u16* vr = vs + j * 128 + hi * 8;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float vf[8];
      unpack8(*(const uint4*)(vr + c * 16), vf);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[c][e] = fmaf(p, vf[e], acc[c][e]);
    }
  }
  const float inv = 1.0f / l;

  if (!valid) return;
  u16* op = out + (long long)b * o_bstride + (long long)row * ld_o + (long long)h * 128 + hi * 8;
  if (FUSED) {
    // the hand-over of add_scaled_kernel on the bf16 term: the product is rounded to bf16 BEFORE it is added, no contraction
#pragma clang fp contract(off)
    const float s = scale[(long long)b * scale_bstride];
    uint4 xr[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) xr[c] = *(const uint4*)(op + c * 16);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float fx[8];
      unpack8(xr[c], fx);
#pragma unroll
      for (int e = 0; e < 8; ++e) fx[e] += rbf(rbf(acc[c][e] * inv) * s);
      *(uint4*)(op + c * 16) = pack8(fx);
    }
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = acc[c][e] * inv;
      *(uint4*)(op + c * 16) = pack8(o);
    }
  }
}

}  // namespace

int fluxmi_k_ip_attention(const void* qkv, long long ld_qkv, long long qkv_bstride, const void* qn_scale, const void* k_ip, const void* v_ip,
                          long long kv_bstride, void* out, long long ld_o, long long o_bstride, const float* scale, long long scale_bstride,
                          int B, int rows, int heads, int Nk, hipStream_t s) {
  FLUXMI_REQUIRE(qkv && qn_scale && k_ip && v_ip && out, "ip_attention: NULL argument");
  FLUXMI_REQUIRE(Nk >= 1 && Nk <= IP_MAX_NK, "ip_attention: Nk = %d outside 1..%d", Nk, IP_MAX_NK);
  FLUXMI_REQUIRE(B >= 0 && B <= 65535 && rows >= 0 && heads >= 1 && heads <= 65535, "ip_attention: bad shape B=%d rows=%d heads=%d", B, rows, heads);
  const long long hd = (long long)heads * 128;
  FLUXMI_REQUIRE(ld_qkv >= hd && ld_o >= hd && ld_qkv % 8 == 0 && ld_o % 8 == 0, "ip_attention: row strides %lld / %lld (>= heads * 128 = %lld, "
                 "multiples of 8)", ld_qkv, ld_o, hd);
  FLUXMI_REQUIRE(qkv_bstride % 8 == 0 && o_bstride % 8 == 0 && kv_bstride % 8 == 0 && scale_bstride >= 0 &&
                 (B <= 1 || (qkv_bstride >= 0 && o_bstride >= (long long)(rows - 1) * ld_o + hd && kv_bstride >= 0)),
                 "ip_attention: batch strides %lld / %lld / %lld (multiples of 8; the output windows of two samples must not overlap)", qkv_bstride,
                 o_bstride, kv_bstride);
  FLUXMI_REQUIRE((uintptr_t)qkv % 16 == 0 && (uintptr_t)qn_scale % 16 == 0 && (uintptr_t)k_ip % 16 == 0 && (uintptr_t)v_ip % 16 == 0 &&
                 (uintptr_t)out % 16 == 0, "ip_attention: every pointer must be 16-byte aligned");
  if (!B || !rows) return 0;
  const dim3 grid((unsigned)((rows + IP_ROWS - 1) / IP_ROWS), (unsigned)heads, (unsigned)B);
  const size_t lds = (size_t)Nk * (512 + IP_ROWS * 4);  // <= 64 KiB at Nk = 64
  if (scale)
    hipLaunchKernelGGL(ip_attention_kernel<true>, grid, dim3(256), lds, s, (const u16*)qkv, ld_qkv, qkv_bstride, (const u16*)qn_scale,
                       (const u16*)k_ip, (const u16*)v_ip, kv_bstride, (u16*)out, ld_o, o_bstride, scale, scale_bstride, rows, heads, Nk);
  else
    hipLaunchKernelGGL(ip_attention_kernel<false>, grid, dim3(256), lds, s, (const u16*)qkv, ld_qkv, qkv_bstride, (const u16*)qn_scale,
                       (const u16*)k_ip, (const u16*)v_ip, kv_bstride, (u16*)out, ld_o, o_bstride, scale, scale_bstride, rows, heads, Nk);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}
