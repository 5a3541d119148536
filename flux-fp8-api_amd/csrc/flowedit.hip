// fluxmi -- FlowEdit (Kulikov et al. 2024, Algorithm 1): the update kernel of inversion-free text-guided editing.
//
// The image stream holds 2B samples: sample b is the SOURCE branch of image b (source prompt, input zs), sample B + b its TARGET branch
// (target prompt, input zt).  Unlike the guided step, the two halves hold DIFFERENT latents, and the state that is stepped -- the edit state
// z -- lives beside the stream.  One kernel does both halves of the algorithm's inner loop:
//   update   (STEP only) with vs = pred[b], vt = pred[B + b] and row j = *step of coef [n][4] = {w, dt, tn, 1 - tn}, ctl [n][2] = {first, apply}:
//              d   = bf16(vt - vs)
//              acc = (first ? 0 : acc) + w * float(d)                 fp32, product and sum each rounded (no fma)
//              apply:  D = bf16(acc);  m = bf16(dt * D);  z' = bf16(z + m), stored;    else acc is stored
//   coupling at time t (STEP: tn of the row; else the launch argument) with n = bf16(the Philox normal of (ids[b], eval, element)):
//              zs = bf16(bf16((1 - t) * x0) + bf16(t * n));   zt = bf16(bf16(z' + zs) - x0)
//            zs -> img[b], zt -> img[B + b].  eval = *step + 1 + *eval_offset (STEP) or the launch argument.
// -- the torch expressions on bf16 tensors with fp32 scalars, one rounding per operation.  first && apply (one evaluation per step, FLUX's
// setting): acc never touches memory and may be NULL.  One thread owns one 16-byte vector = 8 consecutive elements = two Philox blocks;
// every read of a vector precedes its writes; z, x0 and acc are dense [B, rows, C] like each half of img and pred (v1 has neither
// reference rows nor conditioning channels, so the vector index is the offset in all of them).  No LDS, no atomics.
#include "common.h"
#include "fluxmi_internal.h"
#include "philox.h"
#include "stream_view.h"

namespace {

template <bool STEP>
__global__ void __launch_bounds__(256) flowedit_kernel(u16* __restrict__ img, const u16* __restrict__ pred, u16* __restrict__ z,
                                                       float* __restrict__ acc, const u16* __restrict__ x0, const float* __restrict__ coef,
                                                       const int* __restrict__ ctl, const int* __restrict__ step,
                                                       const unsigned* __restrict__ ids, const int* __restrict__ eval_offset, float t_arg,
                                                       float omt_arg, unsigned eval_arg, unsigned n_vec, unsigned vec_per_sample,
                                                       long long half) {
  // every product is rounded before it is added (euler_kernel has the story of the fused bf16 multiply-add): no contraction here
#pragma clang fp contract(off)
  float w = 0.f, dt = 0.f, t = t_arg, omt = omt_arg;
  bool first = true, apply = true;
  unsigned eval = eval_arg;
  if (STEP) {
    const int i = step ? *step : 0;
    w = coef[4 * i]; dt = coef[4 * i + 1]; t = coef[4 * i + 2]; omt = coef[4 * i + 3];
    first = ctl[2 * i] != 0;
    apply = ctl[2 * i + 1] != 0;
    eval = (unsigned)i + 1u + (unsigned)(eval_offset ? *eval_offset : 0);
  }
  // the row is uniform over the launch: so is every branch below.  acc == nullptr with a row that needs it is refused by the callers that
  // can see the row (fluxmi_flowedit_step, the engine); here it only keeps the access from happening
  const bool acc_rd = STEP && !first && acc != nullptr, acc_wr = STEP && !apply && acc != nullptr;
  for (unsigned v = blockIdx.x * blockDim.x + threadIdx.x; v < n_vec; v += gridDim.x * blockDim.x) {
    const long long o = (long long)v * 8;
    float fz[8], f0[8], zn[8], fs[8], ft[8];
    alignas(16) float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const uint4 zraw = *(const uint4*)(z + o);
    unpack8(zraw, fz);
    unpack8(*(const uint4*)(x0 + o), f0);
    if (STEP) {
      float vs[8], vt[8];
      unpack8(*(const uint4*)(pred + o), vs);
      unpack8(*(const uint4*)(pred + half + o), vt);
      if (acc_rd) {
        *(float4*)a = *(const float4*)(acc + o);
        *(float4*)(a + 4) = *(const float4*)(acc + o + 4);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = rbf(vt[j] - vs[j]);
        const float p = (w * d);
        a[j] = ((first ? 0.f : a[j]) + p);
        if (apply) fz[j] = rbf(fz[j] + rbf(dt * rbf(a[j])));
      }
    }
    const unsigned b = v / vec_per_sample;
    philox_normal8(ids + 4 * b, v - b * vec_per_sample, eval, zn);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      fs[j] = rbf(rbf(omt * f0[j]) + rbf(t * rbf(zn[j])));
      ft[j] = rbf(rbf(fz[j] + fs[j]) - f0[j]);
    }
    if (STEP && apply) *(uint4*)(z + o) = pack8(fz);
    if (acc_wr) {
      *(float4*)(acc + o) = *(const float4*)a;
      *(float4*)(acc + o + 4) = *(const float4*)(a + 4);
    }
    *(uint4*)(img + o) = pack8(fs);
    *(uint4*)(img + half + o) = pack8(ft);
  }
}

// the shape rules of both entries -> the vector counts
int fe_shape(const char* who, int B, long long img_rows, long long pred_rows, int c_in, int c_out, long long* n_vec, unsigned* vps) {
  FLUXMI_REQUIRE(c_in == c_out && pred_rows == img_rows, "%s: c_in=%d c_out=%d img_rows=%lld pred_rows=%lld: FlowEdit steps the whole stream "
                 "(no Kontext reference rows, no conditioning channels)", who, c_in, c_out, img_rows, pred_rows);
  FLUXMI_REQUIRE(B >= 0 && pred_rows >= 0 && c_out > 0 && c_out % 8 == 0, "%s: bad shape B=%d rows=%lld c_out=%d (c_out %% 8 == 0)", who, B,
                 pred_rows, c_out);
  *n_vec = (long long)B * pred_rows * (c_out / 8);
  FLUXMI_REQUIRE(*n_vec <= 0x7fffffffLL, "%s: %lld vectors exceed the kernel's 32-bit index", who, *n_vec);
  *vps = (unsigned)(pred_rows * (c_out / 8));
  return 0;
}

}  // namespace

int fluxmi_k_flowedit_couple(void* img, const void* z, const void* x0, float t, float one_minus_t, const unsigned* ids, unsigned eval, int B,
                             long long img_rows, long long pred_rows, int c_in, int c_out, hipStream_t s) {
  FLUXMI_REQUIRE(ids, "flowedit_couple: NULL ids (one {key_lo, key_hi, c2, c3} per image)");
  FLUXMI_REQUIRE(img && z && x0, "flowedit_couple: NULL argument");
  long long n_vec;
  unsigned vps;
  FLUXMI_TRY(fe_shape("flowedit_couple", B, img_rows, pred_rows, c_in, c_out, &n_vec, &vps));
  if (n_vec == 0) return 0;
  hipLaunchKernelGGL((flowedit_kernel<false>), dim3(grid_for(n_vec)), dim3(256), 0, s, (u16*)img, (const u16*)nullptr, (u16*)z, (float*)nullptr,
                     (const u16*)x0, (const float*)nullptr, (const int*)nullptr, (const int*)nullptr, ids, (const int*)nullptr, t, one_minus_t,
                     eval, (unsigned)n_vec, vps, n_vec * 8);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}

int fluxmi_k_flowedit_step(void* img, const void* pred, void* z, float* acc, const void* x0, const float* coef, const int* ctl, const int* step,
                           const unsigned* ids, const int* eval_offset, int B, long long img_rows, long long pred_rows, int c_in, int c_out,
                           hipStream_t s) {
  FLUXMI_REQUIRE(ids, "flowedit_step: NULL ids (one {key_lo, key_hi, c2, c3} per image)");
  FLUXMI_REQUIRE(img && pred && z && x0 && coef && ctl, "flowedit_step: NULL argument");
  long long n_vec;
  unsigned vps;
  FLUXMI_TRY(fe_shape("flowedit_step", B, img_rows, pred_rows, c_in, c_out, &n_vec, &vps));
  if (n_vec == 0) return 0;
  hipLaunchKernelGGL((flowedit_kernel<true>), dim3(grid_for(n_vec)), dim3(256), 0, s, (u16*)img, (const u16*)pred, (u16*)z, acc, (const u16*)x0,
                     coef, ctl, step, ids, eval_offset, 0.f, 0.f, 0u, (unsigned)n_vec, vps, n_vec * 8);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}
