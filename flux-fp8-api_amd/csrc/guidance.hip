// fluxmi -- guidance shaping of true classifier-free guidance (gfx950): CFG rescale, adaptive projected guidance (APG), CFG-Zero*.
//
// Every rule, and any mix of one with rescale, is  p_b = alpha_b * c + beta_b * u + gamma_b * r  per image b: c the prompt branch's
// prediction, u the negative branch's, r APG's running difference, and (alpha, beta, gamma) a closed form of nine per-image sums over
// (c, u, r).  Two launches in front of the guided update:
//   moments: per-workgroup partials of the nine sums, fixed order, no atomics (the ownership rule of fb_metric_kernel, elementwise.hip)
//   combine: every workgroup of an image adds the image's partials in fp64 in ascending order and evaluates the formulas in fp64 -- all of
//            them arrive at the same fp32 coefficients -- then writes v = bf16(p) to BOTH halves of pred.
// The guided update kernels then compute d = bf16(v - v) = 0, m = 0, p = v: they step with v as it is, whatever their scale.
// The formulas are stated in include/fluxmi.h (fluxmi_guidance_combine); they are the definition.
#include "common.h"
#include "fluxmi_internal.h"

namespace {
constexpr unsigned GD_VPT = 8;               // 16-byte vectors per thread
constexpr unsigned GD_CHUNK = 256 * GD_VPT;  // vectors per workgroup: 16384 elements of each operand
constexpr int GD_SUMS = 9;                   // Sc, Su, Sr, cc, uu, rr, cu, cr, ur

// Partials of the nine sums over workgroup g's vectors of image b.  A thread walks its (at most) 8 vectors in ascending order, the 8 elements
// of a vector in ascending order: a chain of at most 64 adds per sum.  Then a 6-level xor butterfly inside each wave and (w0 + w1) + (w2 + w3)
// through LDS: 8 levels, every lane of every wave in one fixed order.  Each product and each sum is rounded to fp32 on its own.
template <bool HAS_R>
__global__ void __launch_bounds__(256) guidance_moments_kernel(const u16* __restrict__ pred, const float* __restrict__ r,
                                                               float* __restrict__ part, unsigned n_vec, long long pred_half) {
#pragma clang fp contract(off)
  __shared__ float lds[4][GD_SUMS];
  const unsigned b = blockIdx.y;
  const long long ob = (long long)b * n_vec * 8;
  float a[GD_SUMS];
#pragma unroll
  for (int i = 0; i < GD_SUMS; ++i) a[i] = 0.f;
#pragma unroll
  for (unsigned j = 0; j < GD_VPT; ++j) {
    const unsigned v = blockIdx.x * GD_CHUNK + j * 256 + threadIdx.x;
    if (v < n_vec) {
      const long long o = ob + (long long)v * 8;
      float fc[8], fu[8];
      alignas(16) float fr[8];
      unpack8(*(const uint4*)(pred + o), fc);
      unpack8(*(const uint4*)(pred + pred_half + o), fu);
      if (HAS_R) {
        *(float4*)fr = *(const float4*)(r + o);
        *(float4*)(fr + 4) = *(const float4*)(r + o + 4);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        a[0] = a[0] + fc[k];
        a[1] = a[1] + fu[k];
        a[3] = a[3] + (fc[k] * fc[k]);
        a[4] = a[4] + (fu[k] * fu[k]);
        a[6] = a[6] + (fc[k] * fu[k]);
        if (HAS_R) {
          a[2] = a[2] + fr[k];
          a[5] = a[5] + (fr[k] * fr[k]);
          a[7] = a[7] + (fc[k] * fr[k]);
          a[8] = a[8] + (fu[k] * fr[k]);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < GD_SUMS; ++i) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a[i] = a[i] + __shfl_xor(a[i], off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < GD_SUMS; ++i) lds[threadIdx.x >> 6][i] = a[i];
  }
  __syncthreads();
  if (threadIdx.x < GD_SUMS) {
    const int i = threadIdx.x;
    part[((long long)b * gridDim.x + blockIdx.x) * GD_SUMS + i] = (lds[0][i] + lds[1][i]) + (lds[2][i] + lds[3][i]);
  }
}

// (alpha, beta, gamma, f) of one image from its nine sums, in fp64; params = {s, phi, eta, rho, mu, mode, zero_init, 0}.  mu arrives as the
// caller decided it (0 without an r buffer).
__device__ void guidance_coefficients(const double* S, double n, const float* __restrict__ params, double mu, bool zero, float* out4) {
#pragma clang fp contract(off)
  const double Sc = S[0], Su = S[1], Sr = S[2], cc = S[3], uu = S[4], rr = S[5], cu = S[6], cr = S[7], ur = S[8];
  const double s = params[0], phi = params[1], eta = params[2], rho = params[3];
  const int mode = (int)params[5];
  double al = s, be = 1.0 - s, ga = 0.0;
  if (mode == 2) {
    const double sstar = uu == 0.0 ? 1.0 : cu / uu;
    be = sstar * (1.0 - s);
  } else if (mode == 1) {
    const double dd = cc + uu + mu * mu * rr - 2.0 * cu + 2.0 * mu * cr - 2.0 * mu * ur;
    const double dc = cc - cu + mu * cr;
    const double tau = (rho > 0.0 && dd > 0.0) ? fmin(1.0, rho / sqrt(dd)) : 1.0;
    const double k = cc == 0.0 ? 0.0 : tau * dc / cc;
    al = 1.0 + (s - 1.0) * (tau + (eta - 1.0) * k);
    be = -(s - 1.0) * tau;
    ga = (s - 1.0) * tau * mu;
  }
  double f = 1.0;
  if (phi > 0.0) {
    const double mean_p = (al * Sc + be * Su + ga * Sr) / n;
    const double e_p2 = (al * al * cc + be * be * uu + ga * ga * rr + 2.0 * al * be * cu + 2.0 * al * ga * cr + 2.0 * be * ga * ur) / n;
    const double var_p = e_p2 - mean_p * mean_p;
    const double var_c = fmax(cc / n - (Sc / n) * (Sc / n), 0.0);  // (a constant c: rounding may leave it below 0)
    if (var_p > 0.0) f = phi * sqrt(var_c / var_p) + (1.0 - phi);
    al *= f;
    be *= f;
    ga *= f;
  }
  if (zero) al = be = ga = 0.0;
  out4[0] = (float)al;
  out4[1] = (float)be;
  out4[2] = (float)ga;
  out4[3] = (float)f;
}

// v = bf16((alpha * c + beta * u) + gamma * r) to both halves of pred; mu != 0: r' = (c - u) + mu * r behind all reads of the element.  A term
// whose coefficient is exactly 0.0f is skipped and its buffer not read (solver_step_kernel's rule); the sum starts at the first term present.
// Every workgroup of image b derives the coefficients itself (thread 0, fp64, ascending partials): no workgroup waits for another.
__global__ void __launch_bounds__(256) guidance_combine_kernel(u16* pred, float* r, const float* __restrict__ part,
                                                               const float* __restrict__ params, const int* __restrict__ step,
                                                               const int* __restrict__ step_offset, float* __restrict__ coef_out,
                                                               unsigned n_vec, unsigned n_part, long long pred_half) {
#pragma clang fp contract(off)
  __shared__ float co[4];
  const unsigned b = blockIdx.y;
  const float mu = r ? params[4] : 0.f;
  if (threadIdx.x == 0) {
    double S[GD_SUMS];
    for (int i = 0; i < GD_SUMS; ++i) S[i] = 0.0;
    const float* pb = part + (long long)b * n_part * GD_SUMS;
    for (unsigned g = 0; g < n_part; ++g)
      for (int i = 0; i < GD_SUMS; ++i) S[i] = S[i] + (double)pb[(long long)g * GD_SUMS + i];
    const long long eval = (long long)(step ? *step : 0) + (long long)(step_offset ? *step_offset : 0);
    guidance_coefficients(S, (double)n_vec * 8.0, params, (double)mu, (float)eval < params[6], co);
    if (blockIdx.x == 0 && coef_out) {
      for (int i = 0; i < 4; ++i) coef_out[4 * b + i] = co[i];
    }
  }
  __syncthreads();
  const float al = co[0], be = co[1], ga = co[2];
  const bool upd = mu != 0.f;
  const bool t_c = al != 0.f, t_u = be != 0.f, t_r = ga != 0.f && r != nullptr;
  const bool rd_c = t_c || upd, rd_u = t_u || upd, rd_r = t_r || upd;
  const long long ob = (long long)b * n_vec * 8;
#pragma unroll
  for (unsigned j = 0; j < GD_VPT; ++j) {
    const unsigned v = blockIdx.x * GD_CHUNK + j * 256 + threadIdx.x;
    if (v < n_vec) {
      const long long o = ob + (long long)v * 8;
      float fc[8], fu[8], fo[8];
      alignas(16) float fr[8];
      if (rd_c) unpack8(*(const uint4*)(pred + o), fc);
      if (rd_u) unpack8(*(const uint4*)(pred + pred_half + o), fu);
      if (rd_r) {
        *(float4*)fr = *(const float4*)(r + o);
        *(float4*)(fr + 4) = *(const float4*)(r + o + 4);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float acc = 0.f;
        bool have = false;
        if (t_c) { acc = (al * fc[k]); have = true; }
        if (t_u) { const float t = (be * fu[k]); acc = have ? (acc + t) : t; have = true; }
        if (t_r) { const float t = (ga * fr[k]); acc = have ? (acc + t) : t; have = true; }
        fo[k] = acc;
        if (upd) fr[k] = (fc[k] - fu[k]) + (mu * fr[k]);
      }
      const uint4 ov = pack8(fo);
      *(uint4*)(pred + o) = ov;
      *(uint4*)(pred + pred_half + o) = ov;
      if (upd) {
        *(float4*)(r + o) = *(const float4*)fr;
        *(float4*)(r + o + 4) = *(const float4*)(fr + 4);
      }
    }
  }
}

int guidance_shape(const char* who, int B, long long N, unsigned* n_vec, unsigned* chunks) {
  FLUXMI_REQUIRE(B >= 1 && B <= 32767 && N >= 8 && N % 8 == 0 && N / 8 <= 0x7fffffffLL,
                 "%s: bad shape B=%d N=%lld (1 <= B <= 32767 images; N = pred_rows * c_out per image, a multiple of 8, N / 8 < 2^31)", who, B, N);
  *n_vec = (unsigned)(N / 8);
  *chunks = (*n_vec + GD_CHUNK - 1) / GD_CHUNK;
  return 0;
}
}  // namespace

int fluxmi_k_guidance_moments(const void* pred, const float* r, float* part, int B, long long N, hipStream_t s) {
  unsigned nv, ch;
  FLUXMI_REQUIRE(pred && part, "guidance_moments: NULL argument");
  FLUXMI_TRY(guidance_shape("guidance_moments", B, N, &nv, &ch));
  if (r)
    hipLaunchKernelGGL(guidance_moments_kernel<true>, dim3(ch, B), dim3(256), 0, s, (const u16*)pred, r, part, nv, (long long)B * N);
  else
    hipLaunchKernelGGL(guidance_moments_kernel<false>, dim3(ch, B), dim3(256), 0, s, (const u16*)pred, r, part, nv, (long long)B * N);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}

int fluxmi_k_guidance_combine(void* pred, float* r, const float* part, const float* params, const int* step, const int* step_offset,
                              float* coef_out, int B, long long N, hipStream_t s) {
  unsigned nv, ch;
  FLUXMI_REQUIRE(pred && part && params, "guidance_combine: NULL argument");
  FLUXMI_TRY(guidance_shape("guidance_combine", B, N, &nv, &ch));
  hipLaunchKernelGGL(guidance_combine_kernel, dim3(ch, B), dim3(256), 0, s, (u16*)pred, r, part, params, step, step_offset, coef_out, nv, ch,
                     (long long)B * N);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}
