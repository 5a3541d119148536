// fluxmi -- latent preview (gfx950): the denoised estimate of one model evaluation, projected 16 -> 3 to RGB at latent resolution.
//
// One launch in front of the update of an evaluation (engine.hip, the `euler` lambda of denoise_impl):  x0 = x - t v  per latent channel,
// rgb = bias + M^T x0, quantised to uint8.  Whether the launch writes at all, and into which slot of the ring, is decided on the device from
// the step counter and a control word {every, eval_offset}: one captured graph serves every cadence and every slice of a request.
// The formulas and their fp32 operation order are stated in include/fluxmi.h (fluxmi_latent_preview); they are the definition.
//
// One thread per token: the token's 64 stepped channels are 128 contiguous bytes of x and of pred -- eight 16-byte loads each, every thread a
// whole line -- and its four pixels are two runs of six bytes.  No LDS, no atomics; ~1 MB of traffic per image at 1024^2, so the kernel is
// launch-latency sized like euler_kernel.
#include "common.h"
#include "fluxmi_internal.h"

namespace {
// vector j of a token holds packed columns 8 j .. 8 j + 7 = latent channels 2 j and 2 j + 1, each with its four sub-pixels (column c * 4 + sub)
template <bool GUIDED>
__global__ void __launch_bounds__(256) latent_preview_kernel(const u16* __restrict__ x, const u16* __restrict__ pred, const float* __restrict__ ts,
                                                             const int* __restrict__ step, const float* __restrict__ scale,
                                                             const float* __restrict__ proj, const int* __restrict__ ctl,
                                                             unsigned char* __restrict__ out, int B, long long img_rows, long long pred_rows,
                                                             int c_in, int h, int w) {
#pragma clang fp contract(off)
  const int st = step ? *step : 0;
  const int every = ctl ? ctl[0] : 1;
  const long long g = (long long)(ctl ? ctl[1] : 0) + st;
  if (every <= 0 || g % every != 0) return;
  const int slot = (int)((g / every) % FLUXMI_PREVIEW_SLOTS);
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= pred_rows) return;
  const int b = blockIdx.y;
  const float t = ts[st];
  const float s = GUIDED ? *scale : 0.f;
  const u16* xp = x + ((long long)b * img_rows + r) * c_in;
  const u16* cp = pred + ((long long)b * pred_rows + r) * 64;
  const u16* up = cp + (long long)B * pred_rows * 64;
  float acc[4][3];
#pragma unroll
  for (int sub = 0; sub < 4; ++sub)
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[sub][k] = proj[48 + k];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float fx[8], fc[8], fu[8];
    unpack8(*(const uint4*)(xp + 8 * j), fx);
    unpack8(*(const uint4*)(cp + 8 * j), fc);
    if (GUIDED) unpack8(*(const uint4*)(up + 8 * j), fu);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = 2 * j + (i >> 2), sub = i & 3;
      const float v = GUIDED ? __builtin_fmaf(s, fc[i] - fu[i], fu[i]) : fc[i];
      const float x0 = __builtin_fmaf(-t, v, fx[i]);
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[sub][k] = __builtin_fmaf(proj[3 * c + k], x0, acc[sub][k]);
    }
  }
  const int ty = (int)(r / w), tx = (int)(r % w);
  unsigned char* ob = out + ((long long)slot * B + b) * (4LL * h * w * 3);
#pragma unroll
  for (int sub = 0; sub < 4; ++sub) {
    const int py = sub >> 1, px = sub & 1;
    unsigned char* o = ob + (((long long)(2 * ty + py)) * (2 * w) + (2 * tx + px)) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float q = rintf(__builtin_fmaf(0.5f, acc[sub][k], 0.5f) * 255.f);
      o[k] = (unsigned char)(q > 0.f ? (q < 255.f ? q : 255.f) : 0.f);  // NaN fails q > 0: 0
    }
  }
}
}  // namespace

int fluxmi_k_latent_preview(const void* x, const void* pred, const float* ts, const int* step, const float* scale, const float* proj,
                            const int* ctl, void* out, int B, long long img_rows, long long pred_rows, int c_in, int c_out, int h, int w,
                            hipStream_t s) {
  FLUXMI_REQUIRE(x && pred && ts && proj && out, "latent_preview: NULL argument");
  FLUXMI_REQUIRE(c_out == 64, "latent_preview: c_out = %d (the projection reads 16 latent channels x 4 sub-pixels = 64 packed columns)", c_out);
  FLUXMI_REQUIRE(h >= 1 && w >= 1 && (long long)h * w == pred_rows, "latent_preview: a token grid of %d x %d for %lld predicted rows (h * w must "
                 "equal the rows the update steps)", h, w, pred_rows);
  FLUXMI_REQUIRE(B >= 1 && B <= 32767 && img_rows >= pred_rows && pred_rows <= 0x7fffffffLL / 256 && c_in >= c_out && c_in % 8 == 0,
                 "latent_preview: bad shape B=%d img_rows=%lld pred_rows=%lld c_in=%d (1 <= B <= 32767, img_rows >= pred_rows, c_in >= 64 and a "
                 "multiple of 8)", B, img_rows, pred_rows, c_in);
  FLUXMI_REQUIRE(((uintptr_t)x | (uintptr_t)pred) % 16 == 0, "latent_preview: x and pred must be 16-byte aligned");
  const dim3 grid((unsigned)((pred_rows + 255) / 256), (unsigned)B);
  if (scale)
    hipLaunchKernelGGL(latent_preview_kernel<true>, grid, dim3(256), 0, s, (const u16*)x, (const u16*)pred, ts, step, scale, proj, ctl,
                       (unsigned char*)out, B, img_rows, pred_rows, c_in, h, w);
  else
    hipLaunchKernelGGL(latent_preview_kernel<false>, grid, dim3(256), 0, s, (const u16*)x, (const u16*)pred, ts, step, scale, proj, ctl,
                       (unsigned char*)out, B, img_rows, pred_rows, c_in, h, w);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}
