// fluxmi -- the kernels of the Depth Anything depth estimator (gfx950; modules/depth.py) that the ViT / VAE / upscaler kernels do not cover:
// the DPT decoder's align-corners bilinear resampling on odd-sized NHWC maps, exact GELU / ReLU, the head's 1x1 convolution to one fp32
// channel, and depth -> uint8 control map.  (The patch rows of its rectangular grid are text.hip's fluxmi_patchify_rect, the symmetric-pad
// stride-2 gather of the last reassemble layer vae.hip's fluxmi_im2col3x3_s2.)
// The arithmetic of every function is stated in include/fluxmi.h.  All of them are bandwidth-sized: one thread moves 16 bytes along C, a
// 1-D grid-stride loop with 64-bit indices walks the output, nothing is staged in LDS except the block reductions of the min / max.
//
// unary_kernel            8 columns per thread; a row's tail (cols % 8) and rows whose address or stride is not 16-byte aligned go element
//                         by element.  Nothing outside [0, cols) of a row is read or written.
// resize_bilinear_kernel  one output pixel x 8 channels per thread: four 16-byte loads, the blend in fp32, one 16-byte store.
// depth_head_kernel       one pixel per thread: dot of its C channels with the weight in fp32, + bias, ReLU, an fp32 store.
// minmax_partial_kernel / minmax_final_kernel   per-image min / max of the depth: fixed chunks, a fixed tree, no atomics.
// depth_to_map_kernel     four output pixels (12 bytes) per thread: half-pixel bilinear source, normalise, round, three equal channels.
#include <math.h>

#include "common.h"
#include "fluxmi_internal.h"

namespace {

typedef unsigned char u8;
constexpr int DEPTH_MAX_BLOCKS = 65535 * 16;
inline int grid_for(long long threads) {
  const long long b = (threads + 255) / 256;
  return (int)(b < 1 ? 1 : (b > DEPTH_MAX_BLOCKS ? DEPTH_MAX_BLOCKS : b));
}
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// 0.5 x (1 + erf(x / sqrt 2)) in fp32: aten's GeluKernel (approximate="none") on a bf16 tensor
__device__ __forceinline__ float unary_f(float x, int kind) {
  if (kind == FLUXMI_UNARY_RELU) return x > 0.f ? x : 0.f;
  return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
}

// (no __restrict__: y may be x)
__global__ void __launch_bounds__(256) unary_kernel(const u16* x, u16* y, long long rows, int cols, long long ldx, long long ldy, int kind,
                                                    int vec) {
  const int c8 = (cols + 7) >> 3;
  const long long total = rows * c8;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / c8;
    const int c0 = (int)(i - r * c8) * 8;
    const u16* xr = x + r * ldx + c0;
    u16* yr = y + r * ldy + c0;
    if (vec && c0 + 8 <= cols) {
      float f[8];
      unpack8(*(const uint4*)xr, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = unary_f(f[j], kind);
      *(uint4*)yr = pack8(f);
    } else {
      const int n = cols - c0 < 8 ? cols - c0 : 8;
      for (int j = 0; j < n; ++j) yr[j] = f2bf(unary_f(bf2f(xr[j]), kind));
    }
  }
}

// source index and weight of one axis, align_corners=True: src = fp32(o * scale), i0 = floor, i1 = i0 + 1 unless i0 is the last, l1 = src - i0
__device__ __forceinline__ void ac_source(int o, float scale, int n_in, int& i0, int& i1, float& l1) {
// src is ROUNDED before i0 is taken off it, as torch rounds it: contracted into fma(scale, o, -i0) the weight moves by up to half an ulp
// of src, which breaks the exact bf16 ties of a blend at l = 1/2 the other way (1.4 % of the outputs of a 19 x 23 -> 37 x 41 resize)
#pragma clang fp contract(off)
  const float src = scale * (float)o;
  i0 = (int)src;
  if (i0 > n_in - 1) i0 = n_in - 1;  // o * scale can round up to n_in - 1 + ulp at the last output; never beyond
  i1 = i0 < n_in - 1 ? i0 + 1 : i0;
  l1 = src - (float)i0;
}

__global__ void __launch_bounds__(256) resize_bilinear_kernel(const u16* __restrict__ x, long long ldx, u16* __restrict__ out, long long ldo,
                                                              const u16* __restrict__ add, long long lda, int B, int Hi, int Wi, int Ho, int Wo,
                                                              int C, float sy, float sx) {
  const int c8 = C >> 3;
  const long long total = (long long)B * Ho * Wo * c8;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int cc = (int)(i % c8);
    const long long pix = i / c8;  // (b * Ho + yo) * Wo + xo
    const int xo = (int)(pix % Wo);
    const long long t = pix / Wo;
    const int yo = (int)(t % Ho);
    const long long b = t / Ho;
    int y0, y1, x0, x1;
    float ly, lx;
    ac_source(yo, sy, Hi, y0, y1, ly);
    ac_source(xo, sx, Wi, x0, x1, lx);
    const float hy = 1.0f - ly, hx = 1.0f - lx;
    const u16* xb = x + cc * 8;
    const long long r0 = (b * Hi + y0) * Wi, r1 = (b * Hi + y1) * Wi;
    float a[8], bq[8], c[8], d[8], o[8];
    unpack8(*(const uint4*)(xb + (r0 + x0) * ldx), a);
    unpack8(*(const uint4*)(xb + (r0 + x1) * ldx), bq);
    unpack8(*(const uint4*)(xb + (r1 + x0) * ldx), c);
    unpack8(*(const uint4*)(xb + (r1 + x1) * ldx), d);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float top = hx * a[j] + lx * bq[j], bot = hx * c[j] + lx * d[j];
      o[j] = hy * top + ly * bot;
    }
    if (add) {
      float e[8];
      unpack8(*(const uint4*)(add + pix * lda + cc * 8), e);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = rbf(o[j]) + e[j];
    }
    *(uint4*)(out + pix * ldo + cc * 8) = pack8(o);
  }
}

__global__ void __launch_bounds__(256) depth_head_kernel(const u16* __restrict__ x, long long ldx, int C, const u16* __restrict__ w,
                                                         const u16* __restrict__ bias, float* __restrict__ out, long long n) {
  const float bv = bias ? bf2f(bias[0]) : 0.f;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
    const u16* xp = x + p * ldx;
    float acc = 0.f;
    for (int c0 = 0; c0 < C; c0 += 8) {
      float f[8], g[8];
      unpack8(*(const uint4*)(xp + c0), f);
      unpack8(*(const uint4*)(w + c0), g);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc = __builtin_fmaf(f[j], g[j], acc);
    }
    acc += bv;
    out[p] = acc > 0.f ? acc : 0.f;
  }
}

// ---- depth -> control map ---------------------------------------------------------------------------------------------------------------
constexpr int MM_CHUNK = 4096;  // elements of one image per workgroup of the first reduction launch

__device__ __forceinline__ void block_minmax(float& mn, float& mx, float* red) {
  mx = wave_max(mx);
  mn = -wave_max(-mn);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[wave] = mn; red[4 + wave] = mx; }
  __syncthreads();
  mn = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
  mx = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
}

__global__ void __launch_bounds__(256) minmax_partial_kernel(const float* __restrict__ d, long long ld, long long bs, int h, int w,
                                                             float* __restrict__ part, int nchunks) {
  __shared__ float red[8];
  const long long n = (long long)h * w;
  const long long e0 = (long long)blockIdx.x * MM_CHUNK, e1 = e0 + MM_CHUNK < n ? e0 + MM_CHUNK : n;
  const float* img = d + (long long)blockIdx.y * bs;
  float mn = INFINITY, mx = -INFINITY;
  for (long long e = e0 + threadIdx.x; e < e1; e += 256) {
    const long long y = e / w;
    const float v = img[y * ld + (e - y * w)];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  block_minmax(mn, mx, red);
  if (threadIdx.x == 0) {
    float* p = part + ((long long)blockIdx.y * nchunks + blockIdx.x) * 2;
    p[0] = mn;
    p[1] = mx;
  }
}

// stats[b] = {min, 255 / (max - min), or 0 for a constant image}
__global__ void __launch_bounds__(256) minmax_final_kernel(const float* __restrict__ part, int nchunks, float* __restrict__ stats) {
  __shared__ float red[8];
  const float* p = part + (long long)blockIdx.x * nchunks * 2;
  float mn = INFINITY, mx = -INFINITY;
  for (int k = threadIdx.x; k < nchunks; k += 256) {
    mn = fminf(mn, p[2 * k]);
    mx = fmaxf(mx, p[2 * k + 1]);
  }
  block_minmax(mn, mx, red);
  if (threadIdx.x == 0) {
    stats[2 * blockIdx.x] = mn;
    stats[2 * blockIdx.x + 1] = mx > mn ? 255.0f / (mx - mn) : 0.f;
  }
}

// half-pixel source of one axis (align_corners=False): src = max(scale * (o + 0.5) - 0.5, 0)
__device__ __forceinline__ void hp_source(int o, float scale, int n_in, int& i0, int& i1, float& l1) {
#pragma clang fp contract(off)  // the product and the difference round separately, as the header states (an fma would move the source)
  float src = scale * ((float)o + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = (int)src;
  if (i0 > n_in - 1) i0 = n_in - 1;
  i1 = i0 < n_in - 1 ? i0 + 1 : i0;
  l1 = src - (float)i0;
  if (l1 > 1.f) l1 = 1.f;
}

__global__ void __launch_bounds__(256) depth_to_map_kernel(const float* __restrict__ d, long long ld, long long bs, int h, int w,
                                                           u8* __restrict__ out, long long old, long long obs, int H, int W,
                                                           const float* __restrict__ stats, float sy, float sx) {
  const int xq = (blockIdx.x * 256 + threadIdx.x) * 4, yo = blockIdx.y, b = blockIdx.z;
  if (xq >= W) return;
  const float* img = d + (long long)b * bs;
  float mn = 0.f, sc = 1.f;
  if (stats) { mn = stats[2 * b]; sc = stats[2 * b + 1]; }
  int y0, y1;
  float ly;
  hp_source(yo, sy, h, y0, y1, ly);
  const float hy = 1.0f - ly;
  const float* r0 = img + (long long)y0 * ld;
  const float* r1 = img + (long long)y1 * ld;
  u8 q[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int xo = xq + e < W ? xq + e : W - 1;
    int x0, x1;
    float lx;
    hp_source(xo, sx, w, x0, x1, lx);
    const float hx = 1.0f - lx;
    const float top = hx * r0[x0] + lx * r0[x1], bot = hx * r1[x0] + lx * r1[x1];
    float v = hy * top + ly * bot;
    if (stats) v = (v - mn) * sc;
    v = floorf(v + 0.5f);
    q[e] = (u8)(v > 0.f ? (v < 255.f ? v : 255.f) : 0.f);  // a NaN depth gives 0
  }
  u8* row = out + (long long)b * obs + (long long)yo * old + (long long)xq * 3;
  const int n = W - xq < 4 ? W - xq : 4;
  if (n == 4 && ((uintptr_t)row & 3) == 0) {
    unsigned* r32 = (unsigned*)row;
    r32[0] = q[0] * 0x010101u | (unsigned)q[1] << 24;
    r32[1] = q[1] * 0x0101u | (unsigned)q[2] * 0x01010000u;
    r32[2] = q[2] | (unsigned)q[3] * 0x01010100u;
  } else {
    for (int e = 0; e < n; ++e) row[3 * e] = row[3 * e + 1] = row[3 * e + 2] = q[e];
  }
}

// [B][H][W] pixels of C channels behind one pixel stride
int pixels_ok(const char* who, const char* name, const void* p, long long ld, int C) {
  FLUXMI_REQUIRE(p && aligned16(p), "%s: %s must be a 16-byte aligned device pointer", who, name);
  FLUXMI_REQUIRE(ld >= C && ld % 8 == 0, "%s: %s pixel stride %lld must be a multiple of 8 that holds its %d channels", who, name, ld, C);
  return 0;
}

}  // namespace

int fluxmi_k_unary(const void* x, void* y, long long rows, int cols, long long ld_in, long long ld_out, int kind, hipStream_t s) {
  FLUXMI_REQUIRE(kind == FLUXMI_UNARY_GELU_ERF || kind == FLUXMI_UNARY_RELU, "unary: kind=%d must be FLUXMI_UNARY_GELU_ERF (0) or "
                 "FLUXMI_UNARY_RELU (1)", kind);
  FLUXMI_REQUIRE(rows >= 0 && cols >= 0, "unary: rows=%lld, cols=%d must be >= 0", rows, cols);
  if (rows == 0 || cols == 0) return 0;
  FLUXMI_REQUIRE(x && y, "unary: NULL tensor");
  FLUXMI_REQUIRE(ld_in >= cols && ld_out >= cols, "unary: row strides %lld / %lld are shorter than cols=%d", ld_in, ld_out, cols);
  const int vec = aligned16(x) && aligned16(y) && ld_in % 8 == 0 && ld_out % 8 == 0;
  hipLaunchKernelGGL(unary_kernel, dim3(grid_for(rows * ((cols + 7) / 8))), dim3(256), 0, s, (const u16*)x, (u16*)y, rows, cols, ld_in, ld_out,
                     kind, vec);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}

int fluxmi_k_resize_bilinear(const void* x, long long ldx, void* out, long long ldo, const void* add, long long lda, int B, int Hi, int Wi,
                             int Ho, int Wo, int C, hipStream_t s) {
  FLUXMI_REQUIRE(B >= 1 && Hi >= 1 && Wi >= 1 && Ho >= 1 && Wo >= 1, "resize_bilinear: B=%d, %dx%d -> %dx%d must all be >= 1", B, Hi, Wi, Ho, Wo);
  FLUXMI_REQUIRE(C >= 8 && C % 8 == 0, "resize_bilinear: C=%d must be a multiple of 8", C);
  FLUXMI_TRY(pixels_ok("resize_bilinear", "x", x, ldx, C));
  FLUXMI_TRY(pixels_ok("resize_bilinear", "out", out, ldo, C));
  if (add) FLUXMI_TRY(pixels_ok("resize_bilinear", "add", add, lda, C));
  FLUXMI_REQUIRE(out != x, "resize_bilinear: out must not be x");
  // torch's area_pixel_compute_scale for align_corners=True: (in - 1) / (out - 1) in fp32, 0 for a single output
  const float sy = Ho > 1 ? (float)(Hi - 1) / (float)(Ho - 1) : 0.f, sx = Wo > 1 ? (float)(Wi - 1) / (float)(Wo - 1) : 0.f;
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3(grid_for((long long)B * Ho * Wo * (C / 8))), dim3(256), 0, s, (const u16*)x, ldx, (u16*)out,
                     ldo, (const u16*)add, lda, B, Hi, Wi, Ho, Wo, C, sy, sx);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}

int fluxmi_k_depth_head(const void* x, long long ldx, int C, const void* w, const void* bias, float* out, long long n, hipStream_t s) {
  FLUXMI_REQUIRE(n >= 1 && C >= 8 && C % 8 == 0, "depth_head: n=%lld must be >= 1 and C=%d a multiple of 8", n, C);
  FLUXMI_TRY(pixels_ok("depth_head", "x", x, ldx, C));
  FLUXMI_REQUIRE(w && aligned16(w) && out && ((uintptr_t)out & 3) == 0, "depth_head: w must be 16-byte aligned, out an fp32 device pointer");
  hipLaunchKernelGGL(depth_head_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const u16*)x, ldx, C, (const u16*)w, (const u16*)bias, out, n);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}

int fluxmi_k_depth_to_map(const float* depth, long long ld, long long bs, void* out, long long out_ld, long long out_bs, float* work,
                          long long work_bytes, int B, int h, int w, int H, int W, int normalize, hipStream_t s) {
  FLUXMI_REQUIRE(B >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "depth_to_map: B=%d, %dx%d -> %dx%d must all be >= 1", B, h, w, H, W);
  FLUXMI_REQUIRE(B <= 65535 && H <= 65535, "depth_to_map: B=%d and H=%d must each fit the launch grid's limit of 65535", B, H);
  FLUXMI_REQUIRE(normalize == FLUXMI_DEPTH_MINMAX || normalize == FLUXMI_DEPTH_RAW, "depth_to_map: normalize=%d must be FLUXMI_DEPTH_MINMAX (0) "
                 "or FLUXMI_DEPTH_RAW (1)", normalize);
  FLUXMI_REQUIRE(depth && ((uintptr_t)depth & 3) == 0 && out, "depth_to_map: depth must be an fp32 device pointer, out not NULL");
  FLUXMI_REQUIRE(ld >= w && (B == 1 || bs >= (long long)h * ld), "depth_to_map: depth strides %lld / %lld are shorter than %d columns / %d rows",
                 ld, bs, w, h);
  FLUXMI_REQUIRE(out_ld >= 3LL * W && (B == 1 || out_bs >= (long long)H * out_ld), "depth_to_map: out strides %lld / %lld are shorter than "
                 "3 * %d bytes / %d rows", out_ld, out_bs, W, H);
  float* stats = nullptr;
  if (normalize == FLUXMI_DEPTH_MINMAX) {
    FLUXMI_REQUIRE(work && ((uintptr_t)work & 3) == 0 && work_bytes >= FLUXMI_DEPTH_MAP_WORK_BYTES(B, h, w),
                   "depth_to_map: work must hold FLUXMI_DEPTH_MAP_WORK_BYTES(%d, %d, %d) = %lld bytes (got %lld)", B, h, w,
                   (long long)FLUXMI_DEPTH_MAP_WORK_BYTES(B, h, w), work_bytes);
    const long long nch = ((long long)h * w + MM_CHUNK - 1) / MM_CHUNK;
    FLUXMI_REQUIRE(nch <= 0x7fffffffLL, "depth_to_map: a %dx%d depth has too many reduction chunks", h, w);
    stats = work + (long long)B * nch * 2;
    hipLaunchKernelGGL(minmax_partial_kernel, dim3((unsigned)nch, B), dim3(256), 0, s, depth, ld, bs, h, w, work, (int)nch);
    FLUXMI_LAUNCH_CHECK();
    hipLaunchKernelGGL(minmax_final_kernel, dim3(B), dim3(256), 0, s, (const float*)work, (int)nch, stats);
    FLUXMI_LAUNCH_CHECK();
  }
  // torch's area_pixel_compute_scale for align_corners=False: in / out in fp32
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  hipLaunchKernelGGL(depth_to_map_kernel, dim3((W + 1023) / 1024, H, B), dim3(256), 0, s, depth, ld, bs, h, w, (u8*)out, out_ld, out_bs, H, W,
                     (const float*)stats, sy, sx);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}
