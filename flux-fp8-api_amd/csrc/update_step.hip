// fluxmi -- the update kernels of the denoise loop (gfx950): the launch that ends every step.  The Euler family (plain, guided, masked, on any
// stream layout) is ONE kernel, the table-driven solver update another; both see the stream through stream_view.h.  The Philox generator
// alone (fluxmi_philox_normal) sits beside the solver update that draws from it.
#include "common.h"
#include "fluxmi_internal.h"
#include "philox.h"
#include "stream_view.h"

#include <type_traits>

namespace {

// The Euler step of the flow ODE, with dt = dts[*step] (step == NULL: dts[0]):
//   x' = bf16(x + bf16(dt * v))                                                                        flux_pipeline.py:651
// CFG (true classifier-free guidance): the stream holds 2B samples, sample b the prompt branch and sample B + b the negative branch of the same
// image; v = guided_chain8 of (c = pred[b], u = pred[B + b], s = *scale) -- the torch expression x + dt * (u + s * (c - u)) on bf16 tensors,
// one rounding per operation.  x is read from the prompt half only and x' is written to both, so the halves stay bit-identical.
// BLEND (masked-latent inpainting): blend_tail8 on x' with tn = tnext[*step], om = one_minus_tnext[*step] and, thr != nullptr (differential
// diffusion), th = thr[*step]; x0 / noise / mask are dense like the prompt half of pred.
// PLAIN: the vector index is the stream offset, in 64 bits (fluxmi_euler takes any n); else stream_offset divides the sample and the row out
// and neither Kontext's reference rows nor Fill's conditioning channels are read or written.  With c_out = 64 the c_out / 8 lanes of one row
// touch one contiguous 128-byte segment of img, and every wave reads pred in one contiguous KiB.
//
// Every product is rounded to bf16 BEFORE it is added.  Two products of the blend tail have two bf16-valued factors (m * x1, (1 - m) * p),
// which the compiler may narrow to a bf16 multiply and then, contracting, fuse into the following add as an fma on the unrounded product (it
// did: one operand of the last sum lost its rounding).  So no contraction in any arm; the arms without a blend round every product before
// its add as well -- rbf sits between each multiply and the add that takes it -- so there is nothing there to contract and the pragma
// cannot move their bits.
template <bool CFG, bool PLAIN, bool BLEND>
__global__ void __launch_bounds__(256) euler_kernel(u16* __restrict__ img, const u16* __restrict__ pred, const u16* __restrict__ x0,
                                                    const u16* __restrict__ noise, const u16* __restrict__ mask, const float* __restrict__ dts,
                                                    const float* __restrict__ tnext, const float* __restrict__ one_minus_tnext,
                                                    const float* __restrict__ thr, const int* __restrict__ step,
                                                    const float* __restrict__ scale, const StreamView sv) {
#pragma clang fp contract(off)
  const int i = step ? *step : 0;
  const float dt = dts[i], sc = CFG ? *scale : 0.f;
  const float tn = BLEND ? tnext[i] : 0.f, om = BLEND ? one_minus_tnext[i] : 0.f;
  const bool diff = BLEND && thr != nullptr;
  const float th = diff ? thr[i] : 0.f;
  for (long long v = blockIdx.x * blockDim.x + threadIdx.x; v < sv.n_vec; v += (long long)gridDim.x * blockDim.x) {
    const long long xo = stream_offset<PLAIN>(sv, v), po = v * 8;
    float fx[8], fv[8], fz[8], fn[8], fm[8];
    unpack8(*(const uint4*)(img + xo), fx);
    unpack8(*(const uint4*)(pred + po), fv);
    if (BLEND) {
      unpack8(*(const uint4*)(x0 + po), fz);
      unpack8(*(const uint4*)(noise + po), fn);
      unpack8(*(const uint4*)(mask + po), fm);
    }
    if (CFG) {
      float fu[8];
      unpack8(*(const uint4*)(pred + sv.pred_half + po), fu);
      guided_chain8(fv, fu, sc);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float x1 = fx[j] + rbf(dt * fv[j]);
      fx[j] = BLEND ? rbf(x1) : x1;  // no blend: pack8 is the sum's rounding
    }
    if (BLEND) blend_tail8(fx, fn, fz, fm, tn, om, diff, th);
    const uint4 o = pack8(fx);
    *(uint4*)(img + xo) = o;
    if (CFG) *(uint4*)(img + sv.img_half + xo) = o;
  }
}

// fluxmi_philox_normal: the generator alone, for tests and tools.  out [B][vec_per_sample * 8]: RAW the uint32 words, else the fp32 normals.
template <bool RAW>
__global__ void __launch_bounds__(256) philox_normal_kernel(void* __restrict__ out, const unsigned* __restrict__ ids, unsigned n_vec,
                                                            unsigned vec_per_sample, unsigned eval) {
  for (unsigned v = blockIdx.x * blockDim.x + threadIdx.x; v < n_vec; v += gridDim.x * blockDim.x) {
    const unsigned b = v / vec_per_sample, w = v - b * vec_per_sample;
    const unsigned* id = ids + 4 * b;
    if (RAW) {
      unsigned r[4];
      philox4x32_10(2 * w, eval, id[2], id[3], id[0], id[1], r);
      ((uint4*)out)[2 * (size_t)v] = make_uint4(r[0], r[1], r[2], r[3]);
      philox4x32_10(2 * w + 1, eval, id[2], id[3], id[0], id[1], r);
      ((uint4*)out)[2 * (size_t)v + 1] = make_uint4(r[0], r[1], r[2], r[3]);
    } else {
      float z[8];
      philox_normal8(id, w, eval, z);
      ((float4*)out)[2 * (size_t)v] = make_float4(z[0], z[1], z[2], z[3]);
      ((float4*)out)[2 * (size_t)v + 1] = make_float4(z[4], z[5], z[6], z[7]);
    }
  }
}
// The table-driven solver update (higher-order samplers): ONE linear update whose coefficients are device data, so the
// engine never knows which solver runs.  Row j = *step of coef [n][8] = {cx, cs, c0, c1, c2, ga, gb, 0} and ctl [n][4] = {save_xs, w_slot,
// h1_slot, h2_slot}; per predicted element, v = pred (CFG: guided_chain8),
//   g   = ga * x + gb * v                                                    fp32
//   acc = cx * x + cs * xs + c0 * g + c1 * hist[h1_slot] + c2 * hist[h2_slot]   fp32, left to right
//   x1  = bf16(acc)                                                          (BLEND: then blend_tail8 on x1)
// Every product and every sum is rounded to fp32 on its own: plain * and + under `fp contract(off)` stay unfused (HIP's __fmul_rn /
// __fadd_rn are inline * / + compiled with contraction allowed, and may fuse once inlined: not used here).  A term whose coefficient is exactly
// 0.0f or whose slot is negative is SKIPPED -- its buffer is not read, it may hold anything -- and the sum starts at the first term that
// is present (0 when none is).  After all reads of the element: save_xs stores the pre-update x to xs, w_slot >= 0 stores g to
// hist[w_slot] (which may be a slot just read), x' goes to img (CFG: both halves).  xs bf16 and hist fp32 [2][...] are dense like the prompt
// half of pred; the indexing is euler_kernel's.  The row is uniform over the launch: every branch below is.
// NOISE (fluxmi_solver_step_noise; the stochastic samplers): column 7 of the row is cn, and one last term follows the c2 term,
//   acc = acc + (cn * z),   z = philox_normal8(ids[b], vector within the image, *step + *eval_offset)
// b the IMAGE (CFG: one draw per image, x' goes to both halves as before).  cn == 0.0f: skipped like every absent term -- ids is not
// read, no generator work -- so the result is the NOISE = false kernel's, which ignores column 7.
template <bool CFG, bool PLAIN, bool BLEND, bool NOISE>
__global__ void __launch_bounds__(256) solver_step_kernel(u16* __restrict__ img, const u16* __restrict__ pred, u16* __restrict__ xs,
                                                          float* __restrict__ hist, const float* __restrict__ coef, const int* __restrict__ ctl,
                                                          const u16* __restrict__ x0, const u16* __restrict__ noise, const u16* __restrict__ mask,
                                                          const float* __restrict__ tnext, const float* __restrict__ one_minus_tnext,
                                                          const float* __restrict__ thr, const int* __restrict__ step,
                                                          const float* __restrict__ scale, const StreamView sv,
                                                          const unsigned* __restrict__ ids, const int* __restrict__ eval_offset) {
#pragma clang fp contract(off)
  const int i = step ? *step : 0;
  const float cx = coef[8 * i], cs = coef[8 * i + 1], c0 = coef[8 * i + 2], c1 = coef[8 * i + 3], c2 = coef[8 * i + 4], ga = coef[8 * i + 5],
              gb = coef[8 * i + 6];
  const float cn = NOISE ? coef[8 * i + 7] : 0.f;
  const bool t_n = NOISE && cn != 0.f;
  const unsigned eval = NOISE ? (unsigned)i + (unsigned)(eval_offset ? *eval_offset : 0) : 0u;
  const bool save = ctl[4 * i] != 0;
  // a slot is -1, 0 or 1: anything above is read as 1, so that no table can index past the two slots
  const int ws = min(ctl[4 * i + 1], 1), s1 = min(ctl[4 * i + 2], 1), s2 = min(ctl[4 * i + 3], 1);
  const bool t_x = cx != 0.f, t_s = cs != 0.f, t_g = c0 != 0.f, t_1 = c1 != 0.f && s1 >= 0, t_2 = c2 != 0.f && s2 >= 0;
  const bool need_g = t_g || ws >= 0;
  const unsigned n_vec = (unsigned)sv.n_vec;
  const long long slot = sv.n_vec * 8;
  const float sc = CFG ? *scale : 0.f;
  const float tn = BLEND ? tnext[i] : 0.f, om = BLEND ? one_minus_tnext[i] : 0.f;
  const bool diff = BLEND && thr != nullptr;
  const float th = diff ? thr[i] : 0.f;
  for (unsigned v = blockIdx.x * blockDim.x + threadIdx.x; v < n_vec; v += gridDim.x * blockDim.x) {
    const long long xo = stream_offset<PLAIN>(sv, v), po = (long long)v * 8;
    const uint4 xraw = *(const uint4*)(img + xo);
    float fx[8], fv[8], fs[8], fo[8], zn[8];
    alignas(16) float h1[8], h2[8], g[8];
    unpack8(xraw, fx);
    unpack8(*(const uint4*)(pred + po), fv);
    if (CFG) {
      float fu[8];
      unpack8(*(const uint4*)(pred + sv.pred_half + po), fu);
      guided_chain8(fv, fu, sc);
    }
    if (t_n) {
      const unsigned b = v / sv.vec_per_sample;
      philox_normal8(ids + 4 * b, v - b * sv.vec_per_sample, eval, zn);
    }
    if (t_s) unpack8(*(const uint4*)(xs + po), fs);
    if (t_1) {
      *(float4*)h1 = *(const float4*)(hist + s1 * slot + po);
      *(float4*)(h1 + 4) = *(const float4*)(hist + s1 * slot + po + 4);
    }
    if (t_2) {
      *(float4*)h2 = *(const float4*)(hist + s2 * slot + po);
      *(float4*)(h2 + 4) = *(const float4*)(hist + s2 * slot + po + 4);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float gj = 0.f;
      if (need_g) {
        if (ga != 0.f) gj = (ga * fx[j]);
        if (gb != 0.f) gj = ga != 0.f ? (gj + (gb * fv[j])) : (gb * fv[j]);
      }
      g[j] = gj;
      float acc = 0.f;
      bool have = false;
      if (t_x) { acc = (cx * fx[j]); have = true; }
      if (t_s) { const float t = (cs * fs[j]); acc = have ? (acc + t) : t; have = true; }
      if (t_g) { const float t = (c0 * gj); acc = have ? (acc + t) : t; have = true; }
      if (t_1) { const float t = (c1 * h1[j]); acc = have ? (acc + t) : t; have = true; }
      if (t_2) { const float t = (c2 * h2[j]); acc = have ? (acc + t) : t; have = true; }
      if (t_n) { const float t = (cn * zn[j]); acc = have ? (acc + t) : t; have = true; }
      fo[j] = rbf(acc);
    }
    if (BLEND) {
      float fz[8], fn[8], fm[8];
      unpack8(*(const uint4*)(x0 + po), fz);
      unpack8(*(const uint4*)(noise + po), fn);
      unpack8(*(const uint4*)(mask + po), fm);
      blend_tail8(fo, fn, fz, fm, tn, om, diff, th);
    }
    if (save) *(uint4*)(xs + po) = xraw;
    if (ws >= 0) {
      *(float4*)(hist + ws * slot + po) = *(const float4*)g;
      *(float4*)(hist + ws * slot + po + 4) = *(const float4*)(g + 4);
    }
    const uint4 o = pack8(fo);
    *(uint4*)(img + xo) = o;
    if (CFG) *(uint4*)(img + sv.img_half + xo) = o;
  }
}

// Runtime flags -> template arms, written once: calls f(std::bool_constant<flag0>{}, std::bool_constant<flag1>{}, ...).
template <class F>
void with_arms(F&& f) { f(); }
template <class F, class... Flags>
void with_arms(F&& f, bool flag, Flags... rest) {
  if (flag) with_arms([&](auto... arms) { f(std::true_type{}, arms...); }, rest...);
  else with_arms([&](auto... arms) { f(std::false_type{}, arms...); }, rest...);
}

// the launcher of fluxmi_k_solver_step (ids == NULL: the deterministic kernel, column 7 ignored) and fluxmi_k_solver_step_noise
int solver_step_launch(void* img, const void* pred, void* xs, float* hist, const float* coef, const int* ctl, const void* x0, const void* noise,
                       const void* mask, const float* tnext, const float* one_minus_tnext, const float* thr, const int* step,
                       const float* scale, int B, long long img_rows, long long pred_rows, int c_in, int c_out, const unsigned* ids,
                       const int* eval_offset, hipStream_t s) {
  FLUXMI_REQUIRE(img && pred && xs && hist && coef && ctl, "solver_step: NULL argument");
  FLUXMI_REQUIRE(!x0 || (noise && mask && tnext && one_minus_tnext), "solver_step: NULL argument (x0, noise, mask, tnext and one_minus_tnext go "
                 "together)");
  StreamView sv;
  FLUXMI_TRY(stream_view("solver_step", B, img_rows, pred_rows, c_in, c_out, &sv));
  if (sv.n_vec == 0) return 0;
  with_arms([&](auto cfg, auto plain, auto blend, auto with_noise) {
    hipLaunchKernelGGL((solver_step_kernel<decltype(cfg)::value, decltype(plain)::value, decltype(blend)::value, decltype(with_noise)::value>),
                       dim3(grid_for(sv.n_vec)), dim3(256), 0, s, (u16*)img, (const u16*)pred, (u16*)xs, hist, coef, ctl, (const u16*)x0,
                       (const u16*)noise, (const u16*)mask, tnext, one_minus_tnext, thr, step, scale, sv, ids, eval_offset);
  }, scale != nullptr, sv.plain, x0 != nullptr, ids != nullptr);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}

// the launch of every Euler arm on a filled view: scale != NULL is CFG, x0 != NULL is BLEND
int euler_launch(void* img, const void* pred, const void* x0, const void* noise, const void* mask, const float* dts, const float* tnext,
                 const float* one_minus_tnext, const float* thr, const int* step, const float* scale, const StreamView& sv, hipStream_t s) {
  if (sv.n_vec == 0) return 0;
  with_arms([&](auto cfg, auto plain, auto blend) {
    hipLaunchKernelGGL((euler_kernel<decltype(cfg)::value, decltype(plain)::value, decltype(blend)::value>), dim3(grid_for(sv.n_vec)), dim3(256),
                       0, s, (u16*)img, (const u16*)pred, (const u16*)x0, (const u16*)noise, (const u16*)mask, dts, tnext, one_minus_tnext, thr,
                       step, scale, sv);
  }, scale != nullptr, sv.plain, x0 != nullptr);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// the flat stream: any n % 8 == 0, the PLAIN arm's 64-bit index (no shape to state, no 32-bit limit)
int fluxmi_k_euler(void* img, const void* pred, const float* dts, const int* step, long long n, hipStream_t s) {
  FLUXMI_REQUIRE(n % 8 == 0, "euler: n must be a multiple of 8");
  StreamView sv = {};
  sv.n_vec = n / 8;
  sv.plain = true;
  return euler_launch(img, pred, nullptr, nullptr, nullptr, dts, nullptr, nullptr, nullptr, step, nullptr, sv, s);
}
int fluxmi_k_euler_step(const char* who, void* img, const void* pred, const void* x0, const void* noise, const void* mask, const float* dts,
                        const float* tnext, const float* one_minus_tnext, const float* thr, const int* step, const float* scale, int B,
                        long long img_rows, long long pred_rows, int c_in, int c_out, hipStream_t s) {
  StreamView sv;
  FLUXMI_TRY(stream_view(who, B, img_rows, pred_rows, c_in, c_out, &sv));
  return euler_launch(img, pred, x0, noise, mask, dts, tnext, one_minus_tnext, thr, step, scale, sv, s);
}
int fluxmi_k_cfg_euler(void* img, const void* pred, const float* dts, const int* step, const float* scale, int B, long long img_rows,
                       long long pred_rows, int c_in, int c_out, hipStream_t s) {
  FLUXMI_REQUIRE(img && pred && dts && scale, "cfg_euler: NULL argument");
  return fluxmi_k_euler_step("cfg_euler", img, pred, nullptr, nullptr, nullptr, dts, nullptr, nullptr, nullptr, step, scale, B, img_rows, pred_rows,
                             c_in, c_out, s);
}
int fluxmi_k_blend_euler(void* img, const void* pred, const void* x0, const void* noise, const void* mask, const float* dts, const float* tnext,
                         const float* one_minus_tnext, const float* thr, const int* step, const float* scale, int B, long long img_rows,
                         long long pred_rows, int c_in, int c_out, hipStream_t s) {
  FLUXMI_REQUIRE(img && pred && x0 && noise && mask && dts && tnext && one_minus_tnext, "blend_euler: NULL argument");
  return fluxmi_k_euler_step("blend_euler", img, pred, x0, noise, mask, dts, tnext, one_minus_tnext, thr, step, scale, B, img_rows, pred_rows, c_in,
                             c_out, s);
}
int fluxmi_k_solver_step(void* img, const void* pred, void* xs, float* hist, const float* coef, const int* ctl, const void* x0, const void* noise,
                         const void* mask, const float* tnext, const float* one_minus_tnext, const float* thr, const int* step,
                         const float* scale, int B, long long img_rows, long long pred_rows, int c_in, int c_out, hipStream_t s) {
  return solver_step_launch(img, pred, xs, hist, coef, ctl, x0, noise, mask, tnext, one_minus_tnext, thr, step, scale, B, img_rows, pred_rows,
                            c_in, c_out, nullptr, nullptr, s);
}
// ids is read by the kernel only where a row's cn != 0, but which row runs is device data: the host cannot tell, so it is always required
int fluxmi_k_solver_step_noise(void* img, const void* pred, void* xs, float* hist, const float* coef, const int* ctl, const void* x0,
                               const void* noise, const void* mask, const float* tnext, const float* one_minus_tnext, const float* thr,
                               const int* step, const float* scale, int B, long long img_rows, long long pred_rows, int c_in, int c_out,
                               const unsigned* ids, const int* eval_offset, hipStream_t s) {
  FLUXMI_REQUIRE(ids, "solver_step_noise: NULL ids (one {key_lo, key_hi, c2, c3} per image; fluxmi_solver_step is the update without noise)");
  return solver_step_launch(img, pred, xs, hist, coef, ctl, x0, noise, mask, tnext, one_minus_tnext, thr, step, scale, B, img_rows, pred_rows,
                            c_in, c_out, ids, eval_offset, s);
}
int fluxmi_k_philox_normal(void* out, const unsigned* ids, int B, long long n_per_image, unsigned eval, int raw, hipStream_t s) {
  FLUXMI_REQUIRE(out && ids, "philox_normal: NULL argument");
  FLUXMI_REQUIRE(B >= 0 && n_per_image >= 0 && n_per_image % 8 == 0 && (raw == 0 || raw == 1),
                 "philox_normal: bad shape B=%d n_per_image=%lld raw=%d (n_per_image a multiple of 8, raw 0 or 1)", B, n_per_image, raw);
  const long long n_vec = (long long)B * (n_per_image / 8);
  FLUXMI_REQUIRE(n_vec <= 0x7fffffffLL, "philox_normal: %lld vectors exceed the kernel's 32-bit index", n_vec);
  if (n_vec == 0) return 0;
  if (raw)
    hipLaunchKernelGGL((philox_normal_kernel<true>), dim3(grid_for(n_vec)), dim3(256), 0, s, out, ids, (unsigned)n_vec,
                       (unsigned)(n_per_image / 8), eval);
  else
    hipLaunchKernelGGL((philox_normal_kernel<false>), dim3(grid_for(n_vec)), dim3(256), 0, s, out, ids, (unsigned)n_vec,
                       (unsigned)(n_per_image / 8), eval);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}
