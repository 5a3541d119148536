// fluxmi -- streaming attention for the autoencoder's mid block (modules/autoencoder.py AttnBlock: ONE head, as wide as the mid block:
// 512 channels in the FLUX VAE, 64 in the tests' small geometry), gfx950.
//
// AutoEncoder._attn's default path builds softmax(Q K^T / sqrt D) V from three launches around a [P, P] bf16 score matrix -- 512 MB at
// 1024^2 (P = 16384), 8 GiB at 2048^2.  This kernel walks the keys in tiles of FLUXMI_VAE_ATTN_KEY_TILE = 64 with a running row maximum
// and row sum, so nothing quadratic in P is ever stored.  Arithmetic (the contract of include/fluxmi.h, restated by tests/vae_attention_ref.py):
//   s_ij  fp32 MFMA sum of bf16 products;   t_ij = s_ij * c,  c = fp32(log2 e / sqrt D)
//   per key tile:  m' = max(m, max_j t_ij) (exact),  alpha = exp2(m - m'),  O *= alpha, l *= alpha (fp32; alpha == 1 leaves the bits alone)
//                  p_ij = exp2(t_ij - m') fp32,  l += sum_j p_ij (fp32),  O += bf16(p) V  (MFMA, fp32 accumulation)
//   out = bf16(O / l + v_bias)          one rounding; keys >= P have p == 0 exactly
// No deferred maximum, no pending P: a tile's P is rounded once, after that tile's maximum is final.
//
// Shape.  One workgroup = 4 waves = 64 query rows, grid (ceil(P / 64), B): 256 workgroups at P = 16384, one per CU.  Both products are
// "swapped" (text.hip): S^T = K Q^T and O^T = V^T P^T on the 32x32x16 bf16 MFMA, so a lane's accumulator column is ONE query (lane & 31)
// and the running max / sum / rescale factor are per-lane scalars.  Wave w = (kh, qh) = (w & 1, w >> 1):
//   scores   the 32 keys kh of the tile against the 32 queries qh over all of D: D/16 MFMAs; its Q^T operand (D/8 registers) is loaded once
//   softmax  tile max of a query: 16 accumulator entries, the other lane half (one cross-lane move), the other kh wave (LDS, barrier 1);
//            bf16 P^T -> LDS [query][key] (9 KiB per parity), barrier 2
//   P V      the D/2 output channels kh of the 32 queries qh: D/64 accumulator tiles (128 registers at D = 512), D/16 MFMAs per tile;
//            A operand = 16 bytes of a V^T row straight from global memory, B operand = 16 bytes of P^T from LDS
// so the O rescale factor a wave needs is the one it computed itself.  K and V^T tiles are not staged in LDS: every element is read by two
// waves of the workgroup and by every workgroup of the launch at about the same time, i.e. from L2.  The LDS buffers alternate by tile parity,
// which makes two barriers per tile enough: a wave can run ahead by at most one barrier, and it then writes the other parity.
// Row sums: a lane sums its 16 p of a tile in accumulator order into its own partial l; the four partials of a query (2 lane halves x 2 kh
// waves) are added once at the end, in that fixed order.  Nothing is atomic; a sample's bits depend on that sample alone (blockIdx.y only
// offsets the pointers).
// Addressing: every product with a row or batch stride is 64-bit.
#include "common.h"
#include "fluxmi_internal.h"

namespace {

constexpr int KT = FLUXMI_VAE_ATTN_KEY_TILE;  // keys per tile
constexpr int QR = 64;                        // query rows per workgroup
constexpr int PT_LD = KT + 8;                 // P^T row pitch in LDS (bf16): 144 bytes, rows stay 16-byte aligned
static_assert(KT == 64, "the wave roles below split a tile into two 32-key halves");

struct VaeAttnArgs {
  const u16* q; const u16* k; long long ld_qk, bs_qk;  // [B][Pp][ld_qk]
  const u16* vt; long long ld_vt, bs_vt;               // [B][D][ld_vt]: V transposed (row = channel, column = key)
  u16* out; long long ld_out, bs_out;                  // [B][P][ld_out]
  const u16* v_bias;                                   // [D] or nullptr
  float c;                                             // log2 e / sqrt D
  int P;
};

template <int D>
__global__ void __launch_bounds__(256) vae_attention_kernel(const VaeAttnArgs a) {
  constexpr int NC = D / 16;   // k-steps of the score MFMA
  constexpr int NDB = D / 64;  // 32-channel output tiles per wave
  __shared__ float s_max[2][2][QR];                  // [parity][kh][query]: tile maximum over a wave's 32 keys
  __shared__ __align__(16) u16 s_pt[2][QR][PT_LD];   // [parity][query][key]: bf16 P^T of the tile
  __shared__ float s_sum[2][QR];                     // [kh][query]: row sums at the end
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, half = lane >> 5;
  const int kh = wave & 1, qh = wave >> 1;
  const int qloc = qh * 32 + l31;
  const long long qrow = (long long)blockIdx.x * QR + qloc;  // < Pp: the grid covers ceil(P / 64) * 64 <= Pp rows
  const long long b = blockIdx.y;
  v8bf qf[NC];
  {
    const u16* qp = a.q + b * a.bs_qk + qrow * a.ld_qk + half * 8;
#pragma unroll
    for (int c = 0; c < NC; ++c) qf[c] = *(const v8bf*)(qp + c * 16);
  }
  const u16* kp = a.k + b * a.bs_qk + (long long)(kh * 32 + l31) * a.ld_qk + half * 8;      // + tile * KT * ld_qk
  const u16* vp = a.vt + b * a.bs_vt + (long long)(kh * (D / 2) + l31) * a.ld_vt + half * 8;  // + tile * KT
  const long long k_step = (long long)KT * a.ld_qk;
  v16f o[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
  float m = -3.0e38f, l = 0.f;
  const int ntile = (a.P + KT - 1) / KT;
  for (int kt = 0; kt < ntile; ++kt) {
    const int par = kt & 1;
    // ---- scores of (32 keys kh) x (32 queries qh): acc[r] = key 8*(r/4) + 4*half + r%4 of the half tile, query l31
    v16f acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const v8bf*)(kp + c * 16), qf[c], acc, 0, 0, 0);
    kp += k_step;
    float t[16];
    const int key0 = kt * KT + kh * 32 + 4 * half;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = key0 + 8 * (r >> 2) + (r & 3);
      t[r] = key < a.P ? acc[r] * a.c : -3.0e38f;
    }
    float tm = t[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) tm = fmaxf(tm, t[r]);
    tm = fmaxf(tm, __shfl_xor(tm, 32));
    if (half == 0) s_max[par][kh][qloc] = tm;
    __syncthreads();
    // every tile holds at least one key < P (ntile = ceil(P / 64)), so mn is a real score from the first tile on
    const float mn = fmaxf(m, fmaxf(s_max[par][0][qloc], s_max[par][1][qloc]));
    const float alpha = __builtin_amdgcn_exp2f(m - mn);  // first tile: exp2(-3e38 - mn) = 0 on O = l = 0
    m = mn;
    float p[16], add = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      p[r] = __builtin_amdgcn_exp2f(t[r] - mn);  // masked key: exp2(-3e38 - mn) = 0 exactly
      add += p[r];
    }
    l = l * alpha + add;
    {
      u16* pw = &s_pt[par][qloc][kh * 32 + 4 * half];
#pragma unroll
      for (int g = 0; g < 4; ++g) *(uint2*)(pw + 8 * g) = make_uint2(pack_bf2(p[4 * g], p[4 * g + 1]), pack_bf2(p[4 * g + 2], p[4 * g + 3]));
    }
    __syncthreads();
    // ---- O^T[channels kh][queries qh] = alpha * O^T + V^T P^T.  alpha == 1 (the row maximum did not grow) is the identity: skip it wave-wide
    if (__any(alpha != 1.0f)) {
#pragma unroll
      for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
    }
    const u16* vk = vp + (long long)kt * KT;
#pragma unroll
    for (int ks = 0; ks < KT / 16; ++ks) {
      const v8bf pb = *(const v8bf*)&s_pt[par][qloc][ks * 16 + half * 8];
#pragma unroll
      for (int db = 0; db < NDB; ++db)
        o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const v8bf*)(vk + (long long)(db * 32) * a.ld_vt + ks * 16), pb, o[db], 0, 0, 0);
    }
  }
  // ---- row sum: lane half 0 + lane half 1 of this wave, then kh 0 + kh 1
  l = l + __shfl_xor(l, 32);
  if (half == 0) s_sum[kh][qloc] = l;
  __syncthreads();
  const float lt = s_sum[0][qloc] + s_sum[1][qloc];
  if (qrow >= a.P) return;
  // O^T[d][q]: this lane holds, for its query, d = kh*D/2 + 32*db + 8*(r/4) + 4*half + r%4
  u16* op = a.out + b * a.bs_out + qrow * a.ld_out + kh * (D / 2) + 4 * half;
  const u16* bp = a.v_bias ? a.v_bias + kh * (D / 2) + 4 * half : nullptr;
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = 32 * db + 8 * g;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = o[db][4 * g + e] / lt;
        if (bp) v[e] += bf2f(bp[d + e]);
      }
      *(uint2*)(op + d) = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
    }
}

}  // namespace

int fluxmi_k_vae_attention(const void* q, const void* k, long long ld_qk, long long bs_qk, const void* vt, long long ld_vt, long long bs_vt,
                           void* out, long long ld_out, long long bs_out, const void* v_bias, int D, int P, int Pp, int B, hipStream_t s) {
  FLUXMI_REQUIRE(D == 64 || D == 512, "vae_attention: D=%d must be 64 or 512 (the mid-block widths the kernel is built for)", D);
  FLUXMI_REQUIRE(P >= 1 && Pp >= P && Pp % 64 == 0, "vae_attention: P=%d must be >= 1 and Pp=%d a multiple of 64 that is >= P", P, Pp);
  FLUXMI_REQUIRE(B >= 1 && B <= 65535, "vae_attention: B=%d must be in 1..65535", B);
  FLUXMI_REQUIRE(q && k && vt && out, "vae_attention: q, k, vt and out must not be NULL");
  FLUXMI_REQUIRE(ld_qk % 8 == 0 && bs_qk % 8 == 0 && ld_qk >= D && (B == 1 || bs_qk >= ld_qk * Pp),
                 "vae_attention: q / k strides (ld_qk %% 8, >= D; bs_qk %% 8, >= ld_qk*Pp)");
  FLUXMI_REQUIRE(ld_vt % 8 == 0 && bs_vt % 8 == 0 && ld_vt >= Pp && (B == 1 || bs_vt >= ld_vt * D),
                 "vae_attention: V^T strides (ld_vt %% 8, >= Pp; bs_vt %% 8, >= ld_vt*D)");
  FLUXMI_REQUIRE(ld_out % 8 == 0 && bs_out % 8 == 0 && ld_out >= D && (B == 1 || bs_out >= ld_out * P),
                 "vae_attention: out strides (ld_out %% 8, >= D; bs_out %% 8, >= ld_out*P)");
  FLUXMI_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)vt | (uintptr_t)out | (uintptr_t)v_bias) % 16 == 0,
                 "vae_attention: q, k, vt, out and v_bias must be 16-byte aligned");
  VaeAttnArgs a;
  a.q = (const u16*)q; a.k = (const u16*)k; a.ld_qk = ld_qk; a.bs_qk = bs_qk; a.vt = (const u16*)vt; a.ld_vt = ld_vt; a.bs_vt = bs_vt;
  a.out = (u16*)out; a.ld_out = ld_out; a.bs_out = bs_out; a.v_bias = (const u16*)v_bias; a.P = P;
  a.c = (float)(1.4426950408889634 / sqrt((double)D));
  const dim3 grid((P + QR - 1) / QR, B);
  if (D == 64) hipLaunchKernelGGL(vae_attention_kernel<64>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(vae_attention_kernel<512>, grid, dim3(256), 0, s, a);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}
