// fluxmi -- the counter-based Gaussian generator shared by every kernel that draws noise (update_step.hip: the stochastic samplers'
// solver update and fluxmi_philox_normal; flowedit.hip: FlowEdit's coupling).  Device functions only: each includer inlines the same code,
// so the bits are the same from every kernel.
#pragma once
#include "common.h"

// Counter-based Gaussian noise for the stochastic samplers: Philox4x32-10 (Salmon et al., SC'11; the published
// multipliers and key increments) and Box-Muller.  One call = one 128-bit block = four normals; counter and key are the caller's, so the
// draw is a pure function of them -- no state, no order, the same bits from every kernel that inlines this.
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned w[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0, h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}
// words -> normals: u = ((w_even >> 9) + 0.5) 2^-23 in (0, 1) and t = (w_odd >> 8) 2^-24 in [0, 1), both exact in fp32;
// r = sqrt(-2 log u), (s, c) = sincospi(2 t); z = r c, r s from (w0, w1), then from (w2, w3).  No fast-math, no contraction.
__device__ __forceinline__ void philox_box_muller(const unsigned w[4], float z[4]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float u = ((float)(w[2 * p] >> 9) + 0.5f) * 0x1p-23f;
    const float t = (float)(w[2 * p + 1] >> 8) * 0x1p-24f;
    const float r = sqrtf(-2.f * logf(u));
    float sn, cs;
    sincospif(2.f * t, &sn, &cs);
    z[2 * p] = r * cs;
    z[2 * p + 1] = r * sn;
  }
}
// the eight normals of vector `vec` (elements [8 vec, 8 vec + 8) of an image's dense block): Philox blocks q = 2 vec and 2 vec + 1 of
// counter (q, eval, id[2], id[3]) under key (id[0], id[1])
__device__ __forceinline__ void philox_normal8(const unsigned* __restrict__ id, unsigned vec, unsigned eval, float z[8]) {
  const unsigned k0 = id[0], k1 = id[1], c2 = id[2], c3 = id[3];
  unsigned w[4];
  philox4x32_10(2 * vec, eval, c2, c3, k0, k1, w);
  philox_box_muller(w, z);
  philox4x32_10(2 * vec + 1, eval, c2, c3, k0, k1, w);
  philox_box_muller(w, z + 4);
}
