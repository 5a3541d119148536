// fluxmi -- the stepped image stream as the update kernels see it: ONE description of its shape, ONE map from vector index to stream offset,
// and the two pieces of bf16 arithmetic every update shares (the guided chain, the inpainting blend tail).
//
// img [B, img_rows, c_in] (guided: 2B samples, the negative branches behind the prompt branches) is stepped from pred [B, pred_rows, c_out].
// The prediction may be SHORTER than the stream (FLUX.1 Kontext: the reference-image rows ride behind the noisy rows of each sample) or
// NARROWER (Fill / Depth / Canny: the conditioning channels ride behind the noisy channels of every token), never both; what it does not
// cover is neither read nor written.  One thread owns one 16-byte vector = 8 channels of one token, vectors numbered along the prompt half of
// pred, which is dense -- as is every side operand (x0, noise, mask, xs, hist): vector v of those is at element v * 8.
#pragma once
#include "common.h"
#include "fluxmi_internal.h"

struct StreamView {
  long long n_vec;              // vectors of one half of pred: the launch's work items
  unsigned vec_per_sample, vec_per_row;
  int c_in;
  long long img_bstride;        // elements from one sample of img to the next
  long long img_half, pred_half;  // elements from the prompt half to the negative half (guided forms)
  bool plain;                   // pred is as long and as wide as the stream: the vector index is the offset
};

// The shape rule of every update that takes (B, img_rows, pred_rows, c_in, c_out), and the 32-bit limit of the divides in stream_offset.
inline int stream_view(const char* who, int B, long long img_rows, long long pred_rows, int c_in, int c_out, StreamView* sv) {
  FLUXMI_REQUIRE(B >= 0 && c_out > 0 && c_out % 8 == 0 && c_in % 8 == 0 && c_out <= c_in && pred_rows >= 0 && pred_rows <= img_rows &&
                     (c_in == c_out || pred_rows == img_rows),
                 "%s: bad shape B=%d img_rows=%lld pred_rows=%lld c_in=%d c_out=%d (channels multiples of 8, c_out <= c_in, pred_rows <= "
                 "img_rows, not both shorter and narrower)", who, B, img_rows, pred_rows, c_in, c_out);
  sv->n_vec = (long long)B * pred_rows * (c_out / 8);
  FLUXMI_REQUIRE(sv->n_vec <= 0x7fffffffLL, "%s: %lld vectors exceed the kernel's 32-bit index", who, sv->n_vec);
  sv->vec_per_sample = (unsigned)(pred_rows * (c_out / 8));
  sv->vec_per_row = (unsigned)(c_out / 8);
  sv->c_in = c_in;
  sv->img_bstride = img_rows * c_in;
  sv->img_half = (long long)B * sv->img_bstride;
  sv->pred_half = sv->n_vec * 8;
  sv->plain = c_in == c_out && pred_rows == img_rows;
  return 0;
}

// vector index -> element offset in img.  PLAIN: no division, any 64-bit v; else the sample and the row are divided out in 32 bits.
template <bool PLAIN>
__device__ __forceinline__ long long stream_offset(const StreamView& sv, long long v) {
  if (PLAIN) return v * 8;
  const unsigned u = (unsigned)v, b = u / sv.vec_per_sample, w = u - b * sv.vec_per_sample, r = w / sv.vec_per_row;
  return b * sv.img_bstride + (long long)r * sv.c_in + (w - r * sv.vec_per_row) * 8;
}

// The guided chain (true classifier-free guidance) on eight lanes: c <- bf16(u + bf16(s * bf16(c - u))), the torch expression
// u + s * (c - u) on bf16 tensors with one rounding per operation.
__device__ __forceinline__ void guided_chain8(float* c, const float* u, float s) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 8; ++j) c[j] = rbf(u[j] + rbf(s * rbf(c[j] - u[j])));
}

// The inpainting blend tail on eight lanes: the stepped x1 (bf16-valued) blended with the init latent re-noised to the NEXT time,
//   p  = bf16(bf16(tn * noise) + bf16(om * x0));   x1 <- bf16(bf16(m * x1) + bf16(bf16(1 - m) * p))
// -- the torch expressions tn * noise + om * x0; (1 - m) * p + m * x1 on bf16 tensors, one rounding per operation, scalars fp32.
// diff (differential diffusion): m is replaced by (float(m) > th ? 1 : 0), compared in fp32.
__device__ __forceinline__ void blend_tail8(float* x1, const float* noise, const float* x0, const float* mask, float tn, float om, bool diff,
                                            float th) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float p = rbf(rbf(tn * noise[j]) + rbf(om * x0[j]));
    const float m = diff ? (mask[j] > th ? 1.f : 0.f) : mask[j];
    x1[j] = rbf(rbf(m * x1[j]) + rbf(rbf(1.f - m) * p));
  }
}

// workgroups of `block` threads for a grid-stride loop over work_items, capped (4096 x 256 threads by default)
inline int grid_for(long long work_items, int block = 256, int cap = 256 * 16) {
  long long g = (work_items + block - 1) / block;
  if (g < 1) g = 1;
  return (int)(g > cap ? cap : g);
}
