// fluxmi -- the residual block of the tiny autoencoder (TAEF1; modules/tiny_vae.py), gfx950: relu(conv3(relu(conv2(relu(conv1(x))))) + x), three
// 3x3 convolutions of 64 -> 64 channels (stride 1, zero pad 1, NHWC bf16) in ONE kernel that reads its input once and writes its output once.
// Unfused (three fluxmi_conv3x3_dense launches, an add and a ReLU) the block moves its activation through HBM seven times; here twice.
// The contract is fluxmi_conv3x3_block's comment in include/fluxmi.h.
//
// Tile plan.  One workgroup = 8 waves = a T x T = 16 x 16 output tile (FLUXMI_CONV_BLOCK_TILE) of one image, in three stages on two LDS
// buffers with conv3x3_dense's 144-byte pixel pitch (consecutive pixels land on different 16-byte bank slots):
//   A   22 x 22 pixels: the input halo (zero outside the image)                                                     69 696 bytes
//   B   20 x 20 pixels: m1 = bf16(relu(conv1 + b1)) of stage 1, read by stage 2                                     57 600 bytes
//   A'  18 x 18 pixels: m2 of stage 2, written back over A (18-pixel rows), read by stage 3
//   Wt  2 x [64 cout][64 cin]: ONE tap's weights, double-buffered (below)                                           18 432 bytes
// 145 728 of the CU's 163 840 bytes: one workgroup per CU, two waves per SIMD.  An m1 / m2 pixel that lies OUTSIDE the image is stored as zero
// -- it is the next convolution's padding, not the value the previous convolution would have there.  The skip is re-read from global memory
// (L2: the workgroup staged the same lines at its start) in stage 3's epilogue, since A' has overwritten the tile's centre by then.
//
// Fragments.  Implicit GEMM in upscaler.hip's swapped layout, D^T[cout][pixel] = W[cout][k] X^T[k][pixel] on v_mfma_f32_32x32x16_bf16: a lane's
// accumulator column is one pixel (lane & 31), its 16 registers are output channels in runs of four (8-byte epilogue accesses).  A stage's
// ragged tile (20^2 = 400, 18^2 = 324, 16^2 = 256 pixels) is cut into 32-pixel fragments by LINEAR pixel index p = 32 f + (lane & 31),
// row p / width, column p % width: 13, 11 and 8 fragments, the last one clamped to the tile's last pixel and not stored beyond it.  Linear
// cutting wastes 16 + 28 + 0 pixel columns of 980; cutting by rows would waste 240 + 252.  Wave w owns fragments w and w + 8 (stages 1 and 2:
// 64 accumulator registers; waves 5..7 / 3..7 own one) and fragment w alone in stage 3, both channel tiles each, so a weight fragment read
// from LDS feeds up to four MFMAs.  Recompute factor (400 + 324 + 256) / (3 x 256) = 1.28 in pixels, (16 + 16 + 8) / 24 = 1.67 in fragment
// slots of the slowest wave.
//
// Weights.  72 KB per convolution does not fit beside A and B, and eight waves reading it from L2 per fragment would be 1.5 MB per tile.
// Instead the 27 taps of the three convolutions stream through Wt: while the waves run tap t's 8 or 16 MFMAs from Wt[t & 1], each of the 512
// threads holds the 16 bytes of tap t + 1 it loaded before them, stores them to Wt[(t + 1) & 1] afterwards, and ONE barrier per tap
// publishes them.  A stage's epilogue sits in front of its last tap's barrier, which therefore also publishes m1 / m2.  221 KB of weight
// reads per tile, all from L2.
//
// Summation order of one convolution output: tap (dy, dx), 16-channel k-step, then the MFMA's own order; fixed, no atomics.  blockIdx.z only
// offsets the pointers: a sample's bits depend on that sample alone.  Every product with a pixel stride is 64-bit.
// Compiler figures (hipcc 7.2, gfx950): 108 VGPRs, 42 SGPRs, no scratch, 145 728 B of LDS: occupancy is set by LDS (one workgroup, 8 waves per CU).
// Measured (profiles/tiny_ae.txt): one block at 1024^2 0.42 ms against 0.87 ms for three conv3x3_dense launches, an add and a ReLU.
#include "common.h"
#include "fluxmi_internal.h"

namespace {

constexpr int T = FLUXMI_CONV_BLOCK_TILE;  // output tile edge
constexpr int CH = 64;                     // channels in and out of every convolution
constexpr int PITCH = CH + 8;              // LDS pixel / weight-row pitch (bf16): 144 bytes
constexpr int NW = 8;                      // waves per workgroup
constexpr int NTHR = NW * 64;
constexpr int W0 = T + 6, W1 = T + 4, W2 = T + 2;  // edges of the input halo, the m1 tile and the m2 tile
constexpr int A_ELEMS = W0 * W0 * PITCH, B_ELEMS = W1 * W1 * PITCH, WT_ELEMS = CH * PITCH;
constexpr int LDS_BYTES = (A_ELEMS + B_ELEMS + 2 * WT_ELEMS) * 2;
constexpr int TAPS = 27;  // 3 convolutions x 9
static_assert(T == 16 && NTHR == CH * 8, "one 16-byte weight load per thread per tap; 13 / 11 / 8 fragments over 8 waves");
static_assert(W2 * W2 <= W0 * W0 && LDS_BYTES <= 160 * 1024, "m2 fits over the halo; everything fits one CU");

struct ConvBlockArgs {
  const u16* x; long long ldx;
  const u16* w; const u16* bias;  // [3][64][3][3][64], [3][64]
  u16* out; long long ldo;
  int H, W;
};

__device__ __forceinline__ void unpack4(const uint2 v, float* r) {
  r[0] = __uint_as_float(v.x << 16); r[1] = __uint_as_float(v.x & 0xffff0000u);
  r[2] = __uint_as_float(v.y << 16); r[3] = __uint_as_float(v.y & 0xffff0000u);
}

// this thread's 16 bytes of global tap gt = 9 conv + tap: input channels 8 (tid & 7) .. + 7 of output channel tid >> 3
__device__ __forceinline__ uint4 load_tap(const u16* w, int gt, int tid) {
  const int conv = gt / 9, tap = gt - 9 * conv;
  return *(const uint4*)(w + ((long long)(conv * CH + (tid >> 3)) * 9 + tap) * CH + (tid & 7) * 8);
}
__device__ __forceinline__ void store_tap(u16* s_w, int gt, int tid, const uint4 v) {
  *(uint4*)&s_w[(gt & 1) * WT_ELEMS + (tid >> 3) * PITCH + (tid & 7) * 8] = v;
}

// One convolution of the block on the tile: STAGE 0 reads the halo (src, SW = 22) and writes m1 (dst, 20 x 20), 1 reads m1 and writes m2
// (18 x 18), 2 reads m2 and writes the output pixels.  Ends with the barrier that publishes dst and the next stage's first tap.
template <int STAGE>
__device__ __forceinline__ void block_stage(const ConvBlockArgs& a, const u16* src, u16* dst, u16* s_w, int y0, int x0, long long b) {
  constexpr int SW = W0 - 2 * STAGE, DW = SW - 2, NPX = DW * DW, NFR = (NPX + 31) / 32, NF = NFR > NW ? 2 : 1;
  constexpr int BORDER = 2 - STAGE;  // the destination tile starts BORDER pixels up-left of the output tile
  static_assert(NFR <= NF * NW, "every fragment has a wave");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
  const bool second = NF == 2 && wave + NW < NFR;  // wave-uniform
  int prow[NF], pcol[NF], xs[NF];
  bool valid[NF];
#pragma unroll
  for (int p = 0; p < NF; ++p) {
    const int px = (wave + NW * p) * 32 + l31;
    const int pc = px < NPX ? px : NPX - 1;
    valid[p] = px < NPX;
    prow[p] = pc / DW; pcol[p] = pc - prow[p] * DW;
    xs[p] = (prow[p] * SW + pcol[p]) * PITCH + half * 8;
  }
  v16f acc[2][NF];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int p = 0; p < NF; ++p)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nt][p][r] = 0.f;

  uint4 wn = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll 1
  for (int tap = 0; tap < 9; ++tap) {
    const int gt = STAGE * 9 + tap;
    if (gt + 1 < TAPS) wn = load_tap(a.w, gt + 1, tid);
    const int dy = tap / 3, dx = tap - 3 * dy;
    const u16* wb = s_w + (gt & 1) * WT_ELEMS + l31 * PITCH + half * 8;
    const int toff = (dy * SW + dx) * PITCH;
#pragma unroll
    for (int ks = 0; ks < CH / 16; ++ks) {
      v8bf wf[2];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) wf[nt] = *(const v8bf*)(wb + nt * 32 * PITCH + ks * 16);
#pragma unroll
      for (int p = 0; p < NF; ++p) {
        if (p == 1 && !second) continue;
        const v8bf xf = *(const v8bf*)&src[xs[p] + toff + ks * 16];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[nt][p] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[nt], xf, acc[nt][p], 0, 0, 0);
      }
    }
    if (tap < 8) {
      store_tap(s_w, gt + 1, tid, wn);
      __syncthreads();
    }
  }

  // ---- epilogue: acc[nt][p][r] = channel 32 nt + 8 (r / 4) + 4 half + r % 4 of tile pixel (prow[p], pcol[p])
  const u16* bias = a.bias + STAGE * CH;
#pragma unroll
  for (int p = 0; p < NF; ++p) {
    if ((p == 1 && !second) || !valid[p]) continue;
    const int gy = y0 - BORDER + prow[p], gx = x0 - BORDER + pcol[p];
    const bool inside = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
    if (STAGE == 2 && !inside) continue;
    const long long pix = (b * a.H + gy) * a.W + gx;  // used when inside only
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c = 32 * nt + 8 * g + 4 * half;
        float y[4], r[4];
        unpack4(*(const uint2*)(bias + c), r);
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = __fadd_rn(acc[nt][p][4 * g + e], r[e]);
        if (STAGE == 2) {
          unpack4(*(const uint2*)(a.x + pix * a.ldx + c), r);
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = __fadd_rn(y[e], r[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = y[e] < 0.f ? 0.f : y[e];
        uint2 v = make_uint2(pack_bf2(y[0], y[1]), pack_bf2(y[2], y[3]));
        if (STAGE == 2) {
          *(uint2*)(a.out + pix * a.ldo + c) = v;
        } else {
          if (!inside) v = make_uint2(0u, 0u);  // the next convolution's zero padding
          *(uint2*)&dst[(prow[p] * DW + pcol[p]) * PITCH + c] = v;
        }
      }
  }
  if (STAGE < 2) {
    store_tap(s_w, STAGE * 9 + 9, tid, wn);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(NTHR) conv3x3_block_kernel(const ConvBlockArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char block_lds[];
  u16* s_a = (u16*)block_lds;
  u16* s_b = s_a + A_ELEMS;
  u16* s_w = s_b + B_ELEMS;
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * T, y0 = blockIdx.y * T;
  const long long b = blockIdx.z;
  {
    const u16* xb = a.x + b * a.H * a.W * a.ldx;
    const int v = tid & 7;  // eight lanes cover the 128 bytes of one pixel
#pragma unroll
    for (int it = 0; it < (W0 * W0 + NTHR / 8 - 1) / (NTHR / 8); ++it) {
      const int px = it * (NTHR / 8) + (tid >> 3);
      const int hr = px / W0, hc = px - hr * W0;
      const int gy = y0 - 3 + hr, gx = x0 - 3 + hc;
      uint4 val = make_uint4(0u, 0u, 0u, 0u);
      if (px < W0 * W0 && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) val = *(const uint4*)(xb + ((long long)gy * a.W + gx) * a.ldx + v * 8);
      if (px < W0 * W0) *(uint4*)&s_a[px * PITCH + v * 8] = val;
    }
    store_tap(s_w, 0, tid, load_tap(a.w, 0, tid));
  }
  __syncthreads();
  block_stage<0>(a, s_a, s_b, s_w, y0, x0, b);
  block_stage<1>(a, s_b, s_a, s_w, y0, x0, b);
  block_stage<2>(a, s_a, nullptr, s_w, y0, x0, b);
}

}  // namespace

int fluxmi_k_conv3x3_block(const void* x, long long ldx, const void* w, const void* bias, void* out, long long ldo, int B, int H, int W,
                           hipStream_t s) {
  FLUXMI_REQUIRE(x && w && bias && out, "conv3x3_block: x, w, bias and out must not be NULL");
  FLUXMI_REQUIRE(B >= 1 && H >= 1 && W >= 1, "conv3x3_block: B=%d, H=%d, W=%d must be >= 1", B, H, W);
  FLUXMI_REQUIRE(B <= 65535 && (H + T - 1) / T <= 65535,
                 "conv3x3_block: B=%d and ceil(H / %d)=%d must each fit the launch grid's limit of 65535", B, T, (H + T - 1) / T);
  FLUXMI_REQUIRE(ldx % 8 == 0 && ldx >= CH, "conv3x3_block: ldx=%lld must be a multiple of 8 that is >= %d", ldx, CH);
  FLUXMI_REQUIRE(ldo % 8 == 0 && ldo >= CH, "conv3x3_block: ldo=%lld must be a multiple of 8 that is >= %d", ldo, CH);
  FLUXMI_REQUIRE(((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)out) % 16 == 0,
                 "conv3x3_block: x, w, bias and out must be 16-byte aligned");
  {
    // a workgroup reads the halo of pixels its neighbours write, and re-reads the skip: the two address ranges must not meet
    const long long npx = (long long)B * H * W;
    const uintptr_t xa = (uintptr_t)x, xe = xa + ((npx - 1) * ldx + CH) * 2, oa = (uintptr_t)out, oe = oa + ((npx - 1) * ldo + CH) * 2;
    FLUXMI_REQUIRE(xe <= oa || oe <= xa, "conv3x3_block: out overlaps x (the address ranges of the two pixel buffers must not meet)");
  }
  ConvBlockArgs a;
  a.x = (const u16*)x; a.ldx = ldx; a.w = (const u16*)w; a.bias = (const u16*)bias; a.out = (u16*)out; a.ldo = ldo; a.H = H; a.W = W;
  // per device and cheap: set on every call, since the kernel cannot launch at all without it
  FLUXMI_CHECK_HIP(hipFuncSetAttribute((const void*)conv3x3_block_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
  hipLaunchKernelGGL(conv3x3_block_kernel, dim3((W + T - 1) / T, (H + T - 1) / T, B), dim3(NTHR), (size_t)LDS_BYTES, s, a);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}
