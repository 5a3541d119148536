// fluxmi -- tiled generation (MultiDiffusion, Bar-Tal et al. 2023): the update kernel of a canvas stepped from overlapping
// windows.
//
// The state that is stepped -- the canvas x, bf16 dense [N, Hc, Wc, C], the token grid of the packed latent -- lives beside the image stream.
// The stream holds S = N * ny * nx samples (2S guided: the negative branches behind the prompt branches) of h * w tokens: sample
// s = (n * ny + a) * nx + b is window (a, b) of image n, its token i * w + j canvas token (row0[a] + i, col0[b] + j).  Windows sit on a
// Cartesian grid, so placement and blend weights are separable: Ny fp32 [ny][Hc], Nx fp32 [nx][Wc], normalised per canvas position by the host
// (fluxmi/windows.py) and zero outside their window.  Per canvas element, with dt = dts[*step]:
//   v_k  = pred[s_k]                                                            unguided
//          guided_chain8 (stream_view.h) of (pred[s_k], pred[S + s_k])           guided (scale != NULL)
//   wgt  = Ny[a][r] * Nx[b][c]                                                   fp32, rounded
//   num  = sum over the covering windows, ascending (a, b), of wgt * v_k         fp32, product and sum each rounded (no fma)
//   vbar = bf16(num);   x' = bf16(x + bf16(dt * vbar))                           (euler_kernel's last operation)
//   canvas <- x';  img[s_k] (and img[S + s_k] when guided) <- x' for every covering window
// STEP = false is the last line alone on x: the gather that fills the stream before the first evaluation.  One thread owns one 16-byte
// vector = 8 channels of one canvas token; every read of a vector precedes its writes; a stream element maps to exactly one canvas token, so
// no two threads touch one address.  No LDS, no atomics.
#include "common.h"
#include "fluxmi_internal.h"
#include "stream_view.h"

namespace {

template <bool STEP>
__global__ void __launch_bounds__(256) window_step_kernel(u16* __restrict__ x, u16* __restrict__ img, const u16* __restrict__ pred,
                                                          const float* __restrict__ dts, const int* __restrict__ step,
                                                          const float* __restrict__ scale, const int* __restrict__ row0,
                                                          const int* __restrict__ col0, const float* __restrict__ Ny,
                                                          const float* __restrict__ Nx, unsigned n_vec, int Hc, int Wc, int h, int w, int ny,
                                                          int nx, int vec_per_tok, long long half, bool guided) {
  // every product is rounded before it is added (euler_kernel has the story of the fused bf16 multiply-add): no contraction here
#pragma clang fp contract(off)
  float dt = 0.f, sc = 0.f;
  if (STEP) {
    dt = dts[step ? *step : 0];
    if (guided) sc = *scale;
  }
  const long long C = (long long)vec_per_tok * 8, win_elems = (long long)h * w * C;
  for (unsigned v = blockIdx.x * blockDim.x + threadIdx.x; v < n_vec; v += gridDim.x * blockDim.x) {
    const unsigned tok = v / (unsigned)vec_per_tok, cv = v - tok * (unsigned)vec_per_tok;
    const unsigned rw = tok / (unsigned)Wc, c = tok - rw * (unsigned)Wc;  // rw = n * Hc + r
    const unsigned n = rw / (unsigned)Hc, r = rw - n * (unsigned)Hc;
    const uint4 xraw = *(const uint4*)(x + (long long)v * 8);
    uint4 o = xraw;
    if (STEP) {
      float fx[8], num[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      unpack8(xraw, fx);
      for (int a = 0; a < ny; ++a) {
        const int i = (int)r - row0[a];
        if (i < 0 || i >= h) continue;
        const float wy = Ny[(long long)a * Hc + r];
        for (int b = 0; b < nx; ++b) {
          const int j = (int)c - col0[b];
          if (j < 0 || j >= w) continue;
          const float wgt = wy * Nx[(long long)b * Wc + c];
          const long long po = ((long long)(n * ny + a) * nx + b) * win_elems + ((long long)i * w + j) * C + cv * 8;
          float fv[8];
          unpack8(*(const uint4*)(pred + po), fv);
          if (guided) {
            float fu[8];
            unpack8(*(const uint4*)(pred + half + po), fu);
            guided_chain8(fv, fu, sc);
          }
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const float p = wgt * fv[k];
            num[k] = num[k] + p;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) fx[k] = fx[k] + rbf(dt * rbf(num[k]));
      o = pack8(fx);
      *(uint4*)(x + (long long)v * 8) = o;
    }
    for (int a = 0; a < ny; ++a) {
      const int i = (int)r - row0[a];
      if (i < 0 || i >= h) continue;
      for (int b = 0; b < nx; ++b) {
        const int j = (int)c - col0[b];
        if (j < 0 || j >= w) continue;
        const long long po = ((long long)(n * ny + a) * nx + b) * win_elems + ((long long)i * w + j) * C + cv * 8;
        *(uint4*)(img + po) = o;
        if (guided) *(uint4*)(img + half + po) = o;
      }
    }
  }
}

// the shape rules of both entries -> the canvas's vector count and the elements of one half of the stream
int win_shape(const char* who, int N, int Hc, int Wc, int h, int w, int ny, int nx, int C, bool guided, long long* n_vec, long long* half) {
  FLUXMI_REQUIRE(C > 0 && C % 8 == 0, "%s: C=%d (C %% 8 == 0: one thread owns 8 channels of a token)", who, C);
  FLUXMI_REQUIRE(N >= 0 && Hc >= 1 && Wc >= 1 && h >= 1 && w >= 1 && ny >= 1 && nx >= 1, "%s: bad shape N=%d canvas %d x %d window %d x %d "
                 "grid %d x %d", who, N, Hc, Wc, h, w, ny, nx);
  FLUXMI_REQUIRE(h <= Hc && w <= Wc, "%s: a window of %d x %d tokens leaves the canvas of %d x %d", who, h, w, Hc, Wc);
  // (in double first: the integer products below must not overflow before they are compared)
  const double stream_vec = (double)N * ny * nx * (guided ? 2.0 : 1.0) * h * w * (C / 8), canvas_vec = (double)N * Hc * Wc * (C / 8);
  FLUXMI_REQUIRE(stream_vec <= 2147483647.0 && canvas_vec <= 2147483647.0, "%s: %.0f stream / %.0f canvas vectors exceed the kernel's 32-bit "
                 "index", who, stream_vec, canvas_vec);
  *n_vec = (long long)N * Hc * Wc * (C / 8);
  *half = (long long)N * ny * nx * h * w * C;
  return 0;
}

}  // namespace

int fluxmi_k_window_gather(const void* canvas, void* img, const int* row0, const int* col0, int N, int Hc, int Wc, int h, int w, int ny, int nx,
                           int C, int guided, hipStream_t s) {
  FLUXMI_REQUIRE(row0 && col0, "window_gather: NULL tables (row0 int32 [ny], col0 int32 [nx] on the device)");
  FLUXMI_REQUIRE(canvas && img, "window_gather: NULL argument");
  long long n_vec, half;
  FLUXMI_TRY(win_shape("window_gather", N, Hc, Wc, h, w, ny, nx, C, guided != 0, &n_vec, &half));
  if (n_vec == 0) return 0;
  hipLaunchKernelGGL((window_step_kernel<false>), dim3(grid_for(n_vec)), dim3(256), 0, s, (u16*)canvas, (u16*)img, (const u16*)nullptr,
                     (const float*)nullptr, (const int*)nullptr, (const float*)nullptr, row0, col0, (const float*)nullptr, (const float*)nullptr,
                     (unsigned)n_vec, Hc, Wc, h, w, ny, nx, C / 8, half, guided != 0);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}

int fluxmi_k_window_step(void* canvas, void* img, const void* pred, const float* dts, const int* step, const float* scale, const int* row0,
                         const int* col0, const float* Ny, const float* Nx, int N, int Hc, int Wc, int h, int w, int ny, int nx, int C,
                         hipStream_t s) {
  FLUXMI_REQUIRE(row0 && col0 && Ny && Nx, "window_step: NULL tables (row0 int32 [ny], col0 int32 [nx], Ny fp32 [ny][Hc], Nx fp32 [nx][Wc] on "
                 "the device)");
  FLUXMI_REQUIRE(canvas && img && pred && dts, "window_step: NULL argument");
  long long n_vec, half;
  FLUXMI_TRY(win_shape("window_step", N, Hc, Wc, h, w, ny, nx, C, scale != nullptr, &n_vec, &half));
  if (n_vec == 0) return 0;
  hipLaunchKernelGGL((window_step_kernel<true>), dim3(grid_for(n_vec)), dim3(256), 0, s, (u16*)canvas, (u16*)img, (const u16*)pred, dts, step,
                     scale, row0, col0, Ny, Nx, (unsigned)n_vec, Hc, Wc, h, w, ny, nx, C / 8, half, scale != nullptr);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}

// The placement rules on HOST copies of the tables, shared by the C ABI entries (which read the device tables back) and the engine (which is
// given host tables): every window inside the canvas, every canvas row and column under some window.
int fluxmi_window_check_tables(const char* who, const int* row0, const int* col0, int Hc, int Wc, int h, int w, int ny, int nx) {
  for (int axis = 0; axis < 2; ++axis) {
    const int* p0 = axis ? col0 : row0;
    const int n = axis ? nx : ny, len = axis ? Wc : Hc, win = axis ? w : h;
    const char* name = axis ? "column" : "row";
    int covered_to = 0;  // every position below it is under a window (the tables need not be sorted: repeat until nothing grows)
    for (int k = 0; k < n; ++k)
      FLUXMI_REQUIRE(p0[k] >= 0 && p0[k] <= len - win, "%s: window %s %d at %d leaves the canvas (%d tokens, window %d)", who, name, k, p0[k], len,
                     win);
    for (bool grew = true; grew && covered_to < len;) {
      grew = false;
      for (int k = 0; k < n; ++k)
        if (p0[k] <= covered_to && p0[k] + win > covered_to) { covered_to = p0[k] + win; grew = true; }
    }
    FLUXMI_REQUIRE(covered_to >= len, "%s: canvas %s %d is under no window", who, name, covered_to);
  }
  return 0;
}
