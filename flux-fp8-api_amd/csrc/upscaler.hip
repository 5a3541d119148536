// fluxmi -- the 3x3 convolution of RRDBNet (ESRGAN / Real-ESRGAN; modules/upscaler.py), gfx950: stride 1, zero pad 1, NHWC bf16, on CHANNEL
// WINDOWS of strided pixel buffers, so the five convolutions of a residual dense block run on ONE [B, H, W, nf + 4 gc] buffer: conv k reads
// channels [0, nf + (k-1) gc) and writes [nf + (k-1) gc, nf + k gc) of the same pixels.  No concatenation copy, no channel padding to the
// 64 / 128 multiples fluxmi_conv3x3 needs (3.4x the trunk's FLOPs).  The contract is fluxmi_conv3x3_dense's comment in include/fluxmi.h.
//
// Shape.  Implicit GEMM, "swapped" like vae_attention.hip: D^T[cout][pixel] = W[cout][k] X^T[k][pixel] on the 32x32x16 bf16 MFMA, so a
// lane's accumulator column is ONE output pixel (lane & 31) and its 16 registers are output channels in runs of four: the epilogue reads the
// residuals and stores with 8-byte accesses.  One workgroup = 4 waves = a 16 x 16 pixel tile (FLUXMI_CONV_DENSE_TILE) of one image; wave w
// owns rows 4w .. 4w+3 as two 32-pixel fragments (2 rows x 16 columns each) times Cout32 / 32 channel tiles: 32 or 64 accumulator registers.
// K = 9 Cin is walked in chunks of 64 input channels: the chunk's 18 x 18 halo (zero outside the image; the nearest-2x upsample folded into
// the source index) is staged in LDS once, 144-byte pixel pitch (consecutive pixels land on different 16-byte bank slots), and all nine taps
// read it with ds_read_b128 at shifted pixel offsets.  Weights are not staged: a lane reads its 16 bytes of W[cout][tap][c..c+8) straight
// from global memory -- every workgroup of the launch reads the same <= 221 KB, i.e. from L2 -- and uses them for both pixel fragments.
// 46.6 KB of LDS and 123 / 193 registers (Cout <= 32 / <= 64): three / two workgroups per CU, whose staging and weight latencies overlap each
// other's MFMAs (no software pipeline inside one).  The dy loop stays rolled: fully unrolled, the compiler hoists every weight load (290 registers).
// Summation order of one output: chunk, tap (dy, dx), 16-channel k-step, then the MFMA's own order; fixed, no atomics.  blockIdx.z only
// offsets the pointers: a sample's bits depend on that sample alone.  Every product with a pixel stride is 64-bit.
#include "common.h"
#include "fluxmi_internal.h"

namespace {

constexpr int TS = FLUXMI_CONV_DENSE_TILE;  // output tile edge
constexpr int HW_ = TS + 2;                 // halo edge
constexpr int HALO_PX = HW_ * HW_;
constexpr int CK = 64;                      // input channels per staged chunk
constexpr int PITCH = CK + 8;               // LDS pixel pitch (bf16): 144 bytes
static_assert(TS == 16, "the wave roles below split a 16 x 16 tile into four 4-row bands of two 2 x 16 fragments");

struct ConvDenseArgs {
  const u16* x; long long ldx; int Cin, Hi, Wi, rshift;  // input pixels [B][Hi][Wi], channels [0, Cin)
  const u16* w2; const u16* bias;                        // [Cout32][3][3][Cin], [Cout32] or nullptr
  u16* out; long long ldo; int Cout;
  const u16* r1; long long ldr1; float a1;
  const u16* r2; long long ldr2; float a2;
  float slope; int act;
  int H, W;
};

// four channels c .. c+3 of one pixel; channels >= Cout are not touched
__device__ __forceinline__ void load4(const u16* p, int c, int Cout, float* r) {
  if (c + 4 <= Cout) {
    const uint2 v = *(const uint2*)(p + c);
    r[0] = __uint_as_float(v.x << 16); r[1] = __uint_as_float(v.x & 0xffff0000u);
    r[2] = __uint_as_float(v.y << 16); r[3] = __uint_as_float(v.y & 0xffff0000u);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = c + e < Cout ? bf2f(p[c + e]) : 0.f;
  }
}

template <int NT, int NKS>
__device__ __forceinline__ void conv_chunk(v16f (&acc)[NT][2], const u16* wp, long long w_tile, int Cin, const u16* s_x, int xs) {
#pragma unroll 1
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
  for (int dx = 0; dx < 3; ++dx) {
    const int tap = dy * 3 + dx;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      v8bf wf[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) wf[nt] = *(const v8bf*)(wp + nt * w_tile + tap * Cin + ks * 16);
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const v8bf xf = *(const v8bf*)&s_x[xs + ((2 * p + dy) * HW_ + dx) * PITCH + ks * 16];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt][p] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[nt], xf, acc[nt][p], 0, 0, 0);
      }
    }
  }
}

template <int NT>
__global__ void __launch_bounds__(256, 2) conv3x3_dense_kernel(const ConvDenseArgs a) {
  __shared__ __align__(16) u16 s_x[HALO_PX * PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
  const int x0 = blockIdx.x * TS, y0 = blockIdx.y * TS;
  const long long b = blockIdx.z;
  const u16* xb = a.x + b * a.Hi * a.Wi * a.ldx;
  const int prow = 4 * wave + (l31 >> 4), pcol = l31 & 15;  // fragment p: tile row prow + 2p, tile column pcol
  const int xs = (prow * HW_ + pcol) * PITCH + half * 8;
  const long long w_tile = 32LL * 9 * a.Cin;
  const u16* wp = a.w2 + (long long)l31 * 9 * a.Cin + half * 8;
  v16f acc[NT][2];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nt][p][r] = 0.f;

  for (int c0 = 0; c0 < a.Cin; c0 += CK) {
    const int ck = a.Cin - c0 < CK ? a.Cin - c0 : CK;
    if (c0) __syncthreads();  // every wave is done reading the previous chunk
    {
      const int v = tid & 7;  // eight lanes cover the 128 bytes of one pixel's chunk
#pragma unroll
      for (int it = 0; it < (HALO_PX + 31) / 32; ++it) {
        const int px = it * 32 + (tid >> 3);
        const int hr = px / HW_, hc = px - hr * HW_;
        const int gy = y0 - 1 + hr, gx = x0 - 1 + hc;
        uint4 val = make_uint4(0u, 0u, 0u, 0u);
        const bool inside = px < HALO_PX && v * 8 < ck;
        if (inside && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)
          val = *(const uint4*)(xb + ((long long)(gy >> a.rshift) * a.Wi + (gx >> a.rshift)) * a.ldx + c0 + v * 8);
        if (inside) *(uint4*)&s_x[px * PITCH + v * 8] = val;
      }
    }
    __syncthreads();
    const u16* wc = wp + c0;
    switch (ck >> 4) {
      case 4: conv_chunk<NT, 4>(acc, wc, w_tile, a.Cin, s_x, xs); break;
      case 3: conv_chunk<NT, 3>(acc, wc, w_tile, a.Cin, s_x, xs); break;
      case 2: conv_chunk<NT, 2>(acc, wc, w_tile, a.Cin, s_x, xs); break;
      default: conv_chunk<NT, 1>(acc, wc, w_tile, a.Cin, s_x, xs); break;
    }
  }

  // ---- epilogue: acc[nt][p][r] = channel 32 nt + 8 (r / 4) + 4 half + r % 4 of pixel (prow + 2p, pcol)
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int row = y0 + prow + 2 * p, col = x0 + pcol;
    if (row >= a.H || col >= a.W) continue;
    const long long pix = (b * a.H + row) * a.W + col;
    u16* op = a.out + pix * a.ldo;
    const u16* r1p = a.r1 ? a.r1 + pix * a.ldr1 : nullptr;
    const u16* r2p = a.r2 ? a.r2 + pix * a.ldr2 : nullptr;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c = 32 * nt + 8 * g + 4 * half;
        if (c >= a.Cout) continue;
        float y[4], r[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = acc[nt][p][4 * g + e];
        if (a.bias) {  // [Cout32]: c + 3 is in bounds
          load4(a.bias, c, 32 * NT, r);
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = __fadd_rn(y[e], r[e]);
        }
        if (a.act) {
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = y[e] < 0.f ? __fmul_rn(a.slope, y[e]) : y[e];
        }
        if (r1p) {
          load4(r1p, c, a.Cout, r);
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = __fadd_rn(__fmul_rn(a.a1, y[e]), r[e]);
        }
        if (r2p) {
          load4(r2p, c, a.Cout, r);
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = __fadd_rn(__fmul_rn(a.a2, y[e]), r[e]);
        }
        if (c + 4 <= a.Cout) {
          *(uint2*)(op + c) = make_uint2(pack_bf2(y[0], y[1]), pack_bf2(y[2], y[3]));
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (c + e < a.Cout) op[c + e] = f2bf(y[e]);
        }
      }
  }
}

}  // namespace

int fluxmi_k_conv3x3_dense(const void* x, long long ldx, int Cin, const void* w2, const void* bias, void* out, long long ldo, int Cout,
                           const void* r1, long long ldr1, float a1, const void* r2, long long ldr2, float a2, float slope, int act,
                           int upsample, int B, int H, int W, hipStream_t s) {
  FLUXMI_REQUIRE(x && w2 && out, "conv3x3_dense: x, w2 and out must not be NULL");
  FLUXMI_REQUIRE(Cin >= 16 && Cin <= 256 && Cin % 16 == 0, "conv3x3_dense: Cin=%d must be a multiple of 16 in 16..256", Cin);
  FLUXMI_REQUIRE(Cout >= 1 && Cout <= 64, "conv3x3_dense: Cout=%d must be in 1..64", Cout);
  FLUXMI_REQUIRE(upsample == 1 || upsample == 2, "conv3x3_dense: upsample=%d must be 1 or 2", upsample);
  FLUXMI_REQUIRE(act == 0 || act == 1, "conv3x3_dense: act=%d must be 0 or 1", act);
  FLUXMI_REQUIRE(B >= 1 && H >= 1 && W >= 1, "conv3x3_dense: B=%d, H=%d, W=%d must be >= 1", B, H, W);
  FLUXMI_REQUIRE(upsample == 1 || (H % 2 == 0 && W % 2 == 0), "conv3x3_dense: upsample 2 needs an even output grid (H=%d, W=%d)", H, W);
  FLUXMI_REQUIRE(B <= 65535 && (H + TS - 1) / TS <= 65535,
                 "conv3x3_dense: B=%d and ceil(H / %d)=%d must each fit the launch grid's limit of 65535", B, TS, (H + TS - 1) / TS);
  FLUXMI_REQUIRE(ldx % 8 == 0 && ldx >= Cin, "conv3x3_dense: ldx=%lld must be a multiple of 8 that is >= Cin=%d", ldx, Cin);
  FLUXMI_REQUIRE(ldo % 8 == 0 && ldo >= Cout, "conv3x3_dense: ldo=%lld must be a multiple of 8 that is >= Cout=%d", ldo, Cout);
  FLUXMI_REQUIRE(!r1 || (ldr1 % 8 == 0 && ldr1 >= Cout), "conv3x3_dense: ldr1=%lld must be a multiple of 8 that is >= Cout=%d", ldr1, Cout);
  FLUXMI_REQUIRE(!r2 || (ldr2 % 8 == 0 && ldr2 >= Cout), "conv3x3_dense: ldr2=%lld must be a multiple of 8 that is >= Cout=%d", ldr2, Cout);
  FLUXMI_REQUIRE(r1 || !r2, "conv3x3_dense: r2 is the SECOND residual: it needs r1");
  FLUXMI_REQUIRE(((uintptr_t)x | (uintptr_t)w2 | (uintptr_t)bias | (uintptr_t)out | (uintptr_t)r1 | (uintptr_t)r2) % 16 == 0,
                 "conv3x3_dense: x, w2, bias, out, r1 and r2 must be 16-byte aligned");
  FLUXMI_REQUIRE(out != r1 && out != r2, "conv3x3_dense: out must not overlap a residual");
  ConvDenseArgs a;
  a.x = (const u16*)x; a.ldx = ldx; a.Cin = Cin; a.rshift = upsample == 2 ? 1 : 0; a.Hi = H >> a.rshift; a.Wi = W >> a.rshift;
  a.w2 = (const u16*)w2; a.bias = (const u16*)bias; a.out = (u16*)out; a.ldo = ldo; a.Cout = Cout;
  a.r1 = (const u16*)r1; a.ldr1 = ldr1; a.a1 = a1; a.r2 = (const u16*)r2; a.ldr2 = ldr2; a.a2 = a2;
  a.slope = slope; a.act = act; a.H = H; a.W = W;
  const dim3 grid((W + TS - 1) / TS, (H + TS - 1) / TS, B);
  if (Cout <= 32) hipLaunchKernelGGL(conv3x3_dense_kernel<1>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(conv3x3_dense_kernel<2>, grid, dim3(256), 0, s, a);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}
