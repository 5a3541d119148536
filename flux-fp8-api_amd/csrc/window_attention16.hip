// fluxmi -- 16 x 16 window attention with an indexed relative-position bias, for HAT (modules/hat.py), gfx950: the window self-attention of
// its hybrid attention blocks (256 queries x 256 keys, shift 0 / 8) and its overlapping cross-attention block (OCAB: 256 queries x the
// 24 x 24 = 576 pixels around the window), plus the two small kernels of HAT's channel attention (per-image channel mean; squeeze MLP and
// the block's three-way sum).
//
// HAT computes  roll -> window_partition (q) / nn.Unfold(24, stride 16, padding 4) (k, v) -> softmax(q k^T scale + table[index]) v -> reverse
// -> roll back  with a materialised [windows, heads, 256, 576] score tensor.  Here all of that is ADDRESS ARITHMETIC of one launch, as in
// window_attention.hip, and Unfold's zero padding is a key whose k and v are written as zeros while staging (never read from memory): its
// logit is its bias alone, it takes part in the softmax, and it adds nothing to the numerator.
// Arithmetic (the contract of include/fluxmi.h, restated by tests/hat_ref.py):
//   s = fp32 MFMA sum of the bf16 products q . k over the head's 32 columns;   t = (s * scale + table[index[a][b]][h]) (+ -100 across regions)
//   STREAMED softmax over key tiles of 32: a running maximum m per query; entering a tile, l and O are multiplied by exp(m_old - m_new);
//   p = exp(t - m) fp32, l += p fp32, O += bf16(p) v (MFMA, fp32);   out = bf16(O / l)              one rounding of the output
//
// Shape.  One workgroup = one query window of one image, 8 waves; wave w owns queries 32 w .. 32 w + 31 (two window rows) and WALKS THE HEADS:
// 256 x 576 x 32 per head does not fit registers the way the 64-token kernel's problem does, and all heads' K / V exceed the LDS, so per head
// the workgroup stages that head's neighbourhood once and every wave streams over it.
//   stage    K [key][32] (16-byte chunks XOR-swizzled by (key / 2) % 4: row pitch 64 B with conflict-free 16-byte operand reads and no pad),
//            V^T [32][key] (pitch 580: 290 banks = 34 mod 64, the 8-window kernel's choice), the head's table column (<= 1521 floats).
//            80068 B: two workgroups per CU.  The key's pixel is the rolled window pixel (overlap 0) or window origin - 4 + (kk / 24, kk % 24).
//   scores   both products are "swapped" (S^T = K Q^T, O^T = V^T P^T on v_mfma_f32_32x32x16_bf16), so an accumulator column is ONE query
//            (lane & 31) and m, l, the rescale and 1 / l are per-lane scalars plus one exchange with the other lane half.  Q sits in operand
//            registers for the whole head (loaded from the pixel row), K comes from LDS: two MFMAs per 32-key tile.
//   bias     accumulator entry r of a tile is key 32 kt + 8 (r / 4) + 4 half + r % 4, so the lane's sixteen indices are four 16-byte runs of
//            index row a, read ONCE per (query row, key tile) and prefetched one tile ahead; the table lookups are LDS gathers.
//   mask     key tile kt lies in window rows 2 kt, 2 kt + 1 and entry r in columns 8 ((r / 4) % 2) + 4 half + r % 4: the key's region is
//            (kt >= 4, (r / 4) % 2), the query's (row >= 8, column >= 8), compared only in the last window row / column -- no id table.
//   P V      k-slot (half, j) of step g is DEFINED as key 32 kt + 16 g + 8 (j / 4) + 4 half + j % 4, the eight p a lane already holds in
//            entries 8 g .. 8 g + 7 (a sum over keys does not care about their order): P never leaves its registers.
//   store    O^T[d][query]: four 8-byte stores into the query's source pixel.  Zero-padded head columns give O = 0 exactly.
// Nothing is atomic; blockIdx.y only offsets pointers.  Addresses are 64-bit.  The index entries are trusted (the caller checks them once).
#include "common.h"
#include "fluxmi_internal.h"

namespace {

constexpr int WS = FLUXMI_WINDOW16;                      // window edge
constexpr int NQ = WS * WS;                              // queries per window
constexpr int OV = 4;                                    // OCAB's overlap on each side
constexpr int WE = WS + 2 * OV;                          // edge of the key neighbourhood
constexpr int NK_MAX = WE * WE;                          // 576
constexpr int HD = 32;                                   // padded head width
constexpr int WAVES = NQ / 32;                           // 8: one 32-query tile per wave
constexpr int VT_LD = NK_MAX + 4;                        // V^T row pitch (bf16)
constexpr int TAB_MAX = (WS + WE - 1) * (WS + WE - 1);   // 1521 table rows at most
constexpr int LDS_K = NK_MAX * HD * 2, LDS_VT = HD * VT_LD * 2, LDS_BYTES = LDS_K + LDS_VT + TAB_MAX * 4;
static_assert(WS == 16 && NQ == 256 && LDS_K % 16 == 0 && (LDS_K + LDS_VT) % 16 == 0, "the lane roles below are written for 16 x 16 windows");

struct Win16Args {
  const u16* qkv; long long ld;   // [B][H][W] pixels: q | k | v, each heads * 32 columns
  const float* table;             // [table_rows][heads]
  const int* index;               // [256][Nk]
  u16* out; long long ldo;        // [B][H][W] pixels, heads * 32 columns written
  int H, W, heads, shift, overlap, table_rows;
  float scale;
};

__global__ void __launch_bounds__(WAVES * 64) window_attention16_kernel(const Win16Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char w16_lds[];
  u16* s_k = (u16*)w16_lds;                         // [key][4 swizzled chunks of 8]
  u16* s_vt = (u16*)(w16_lds + LDS_K);              // [HD][VT_LD]
  float* s_tab = (float*)(w16_lds + LDS_K + LDS_VT);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
  const int nwx = a.W / WS;
  const int wy = blockIdx.x / nwx, wx = blockIdx.x - wy * nwx;
  const long long img = (long long)blockIdx.y * a.H * a.W;
  const int we = a.overlap ? WE : WS, Nk = we * we, ntile = Nk / 32;
  const int C = a.heads * HD;
  // pixel of key kk of this window's neighbourhood as a pixel index, or -1 for Unfold's zero padding
  auto key_pixel = [&](int kk) -> long long {
    const int ky = kk / we, kx = kk - ky * we;
    int y = WS * wy + ky, x = WS * wx + kx;
    if (a.overlap) {
      y -= OV;
      x -= OV;
      if (y < 0 || y >= a.H || x < 0 || x >= a.W) return -1;
    } else {
      y += a.shift;
      x += a.shift;
      y -= y >= a.H ? a.H : 0;
      x -= x >= a.W ? a.W : 0;
    }
    return img + (long long)y * a.W + x;
  };
  // the lane's query: token qa of the window, read and written at its source pixel
  const int qa = 32 * wave + l31, qty = qa >> 4, qtx = qa & 15;
  long long qpix;
  {
    int y = WS * wy + qty + a.shift, x = WS * wx + qtx + a.shift;
    y -= y >= a.H ? a.H : 0;
    x -= x >= a.W ? a.W : 0;
    qpix = img + (long long)y * a.W + x;
  }
  const bool last_row = a.shift > 0 && wy == a.H / WS - 1, last_col = a.shift > 0 && wx == nwx - 1;
  const bool q_row_hi = qty >= 8;
  // -100 for the keys of column region 0 / 1 (entry (r / 4) % 2) when the column regions differ
  const bool col_cut0 = last_col && qtx >= 8, col_cut1 = last_col && qtx < 8;
  const int* irow = a.index + (long long)qa * Nk + 4 * half;

  for (int h = 0; h < a.heads; ++h) {
    v8bf qf[2];  // columns 16 s + 8 half .. of the query's head
    {
      const u16* qp = a.qkv + qpix * a.ld + h * HD + 8 * half;
      qf[0] = *(const v8bf*)qp;
      qf[1] = *(const v8bf*)(qp + 16);
    }
    if (h) __syncthreads();  // every wave is done reading the previous head's K, V^T and table
    for (int c = tid; c < Nk * 4; c += WAVES * 64) {
      const int key = c >> 2, ch = c & 3;
      const long long pix = key_pixel(key);
      uint4 kv = make_uint4(0u, 0u, 0u, 0u), vv = kv;
      if (pix >= 0) {
        const u16* p = a.qkv + pix * a.ld + C + h * HD + 8 * ch;
        kv = *(const uint4*)p;
        vv = *(const uint4*)(p + C);
      }
      *(uint4*)(s_k + key * HD + 8 * (ch ^ ((key >> 1) & 3))) = kv;
      const unsigned w[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s_vt[(8 * ch + 2 * j) * VT_LD + key] = (u16)(w[j] & 0xffffu);
        s_vt[(8 * ch + 2 * j + 1) * VT_LD + key] = (u16)(w[j] >> 16);
      }
    }
    for (int i = tid; i < a.table_rows; i += WAVES * 64) s_tab[i] = a.table[(long long)i * a.heads + h];
    __syncthreads();

    float m = -3.0e38f, l = 0.f;  // l: this lane half's part of the sum
    v16f o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    uint4 ix[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) ix[g] = *(const uint4*)(irow + 8 * g);
    for (int kt = 0; kt < ntile; ++kt) {
      uint4 nx[4];
      const int ktn = kt + 1 < ntile ? kt + 1 : kt;
#pragma unroll
      for (int g = 0; g < 4; ++g) nx[g] = *(const uint4*)(irow + 32 * ktn + 8 * g);
      // ---- S^T tile: acc[r] = key 32 kt + 8 (r / 4) + 4 half + r % 4, query l31
      v16f acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const int key = 32 * kt + l31;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const v8bf kf = *(const v8bf*)(s_k + key * HD + 8 * ((2 * s + half) ^ ((key >> 1) & 3)));
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], acc, 0, 0, 0);
      }
      const bool row_cut = last_row && (q_row_hi != (kt >= 4));
      const float mk[2] = {(row_cut || col_cut0) ? -100.f : 0.f, (row_cut || col_cut1) ? -100.f : 0.f};
      const int id[16] = {(int)ix[0].x, (int)ix[0].y, (int)ix[0].z, (int)ix[0].w, (int)ix[1].x, (int)ix[1].y, (int)ix[1].z, (int)ix[1].w,
                          (int)ix[2].x, (int)ix[2].y, (int)ix[2].z, (int)ix[2].w, (int)ix[3].x, (int)ix[3].y, (int)ix[3].z, (int)ix[3].w};
      float mt = -3.0e38f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float t = acc[r] * a.scale + s_tab[id[r]];
        t += mk[(r >> 2) & 1];
        acc[r] = t;
        mt = fmaxf(mt, t);
      }
      mt = fmaxf(mt, __shfl_xor(mt, 32));
      const float mn = fmaxf(m, mt), alpha = __expf(m - mn);
      m = mn;
      l *= alpha;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        o[r] *= alpha;
        const float p = __expf(acc[r] - m);
        acc[r] = p;
        l += p;
      }
      // ---- O^T[d][query] += V^T P^T, two k-steps; k-slot (half, j) = key 32 kt + 16 g + 8 (j / 4) + 4 half + j % 4
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const u16* vr = s_vt + l31 * VT_LD + 32 * kt + 16 * g + 4 * half;
        union { uint2 u[2]; v8bf v; } va;
        va.u[0] = *(const uint2*)vr;
        va.u[1] = *(const uint2*)(vr + 8);
        union { unsigned u[4]; v8bf v; } pb;
#pragma unroll
        for (int j = 0; j < 4; ++j) pb.u[j] = pack_bf2(acc[8 * g + 2 * j], acc[8 * g + 2 * j + 1]);
        o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va.v, pb.v, o, 0, 0, 0);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) ix[g] = nx[g];
    }
    l += __shfl_xor(l, 32);
    // ---- o[r] = O^T[d = 8 (r / 4) + 4 half + r % 4][query l31]
    u16* op = a.out + qpix * a.ldo + h * HD + 4 * half;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = o[4 * g + e] / l;
      *(uint2*)(op + 8 * g) = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
    }
  }
}

// ---- channel attention (HAT's CAB tail): mean over the pixels of each image and channel, then the squeeze MLP and the block's sum.
// channel_partial_kernel: block (chunk, image) sums CM_CHUNK pixels.  Thread (pr, cc) adds the 8 channels of chunk cc over pixels pr, pr + PL, ..
// of the chunk in that order (fp32), the PL partial rows meet in LDS and are added in the order pr = 0, 1, ..: work[image][chunk][channel].
// channel_mean_kernel: block (16 channels, image); run r of 16 adds chunks r, r + 16, .. of a channel in that order (one thread walking
// every chunk is a chain of dependent loads: 59 us at 256 chunks against 10 us for the pixels themselves), the 16 runs are added in the
// order r = 0, 1, .. and divided by P.  No atomics: every sum has ONE order.
constexpr int CM_CHUNK = 256, CM_THREADS = 256, CM_CMAX = 512, CF_CH = 16, CF_RUNS = CM_THREADS / CF_CH;

__global__ void __launch_bounds__(CM_THREADS) channel_partial_kernel(const u16* __restrict__ x, long long ld, float* __restrict__ work,
                                                                     long long P, int C, int nchunk) {
  __shared__ float s_part[CM_THREADS * 8];
  const int C8 = C / 8, PL = CM_THREADS / C8, tid = threadIdx.x;
  const int pr = tid / C8, cc = tid - pr * C8;
  const long long p0 = (long long)blockIdx.x * CM_CHUNK, p1 = p0 + CM_CHUNK < P ? p0 + CM_CHUNK : P;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (pr < PL) {
    const u16* xp = x + ((long long)blockIdx.y * P) * ld + cc * 8;
    for (long long p = p0 + pr; p < p1; p += PL) {
      float v[8];
      unpack8(*(const uint4*)(xp + p * ld), v);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += v[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) s_part[pr * C + cc * 8 + j] = acc[j];
  }
  __syncthreads();
  for (int c = tid; c < C; c += CM_THREADS) {
    float s = 0.f;
    for (int r = 0; r < PL; ++r) s += s_part[r * C + c];
    work[((long long)blockIdx.y * nchunk + blockIdx.x) * C + c] = s;
  }
}

__global__ void __launch_bounds__(CM_THREADS) channel_mean_kernel(const float* __restrict__ work, float* __restrict__ mean, long long P, int C,
                                                                  int nchunk) {
  __shared__ float s_run[CF_RUNS][CF_CH];
  const int cl = threadIdx.x % CF_CH, run = threadIdx.x / CF_CH, c = blockIdx.x * CF_CH + cl;
  float s = 0.f;
  if (c < C) {
    const float* w = work + (long long)blockIdx.y * nchunk * C + c;
    for (int i = run; i < nchunk; i += CF_RUNS) s += w[(long long)i * C];
  }
  s_run[run][cl] = s;
  __syncthreads();
  if (run == 0 && c < C) {
    float t = 0.f;
#pragma unroll
    for (int r = 0; r < CF_RUNS; ++r) t += s_run[r][cl];
    mean[(long long)blockIdx.y * C + c] = t / (float)P;
  }
}

// channel_combine_kernel: every block first recomputes its image's gate (Cs x C + C x Cs products: cheaper than a launch of its own):
//   hid[j] = relu(b1[j] + sum_c w1[j][c] mean[c])  (one wave per j, lanes over c, wave_sum);  g[c] = 1 / (1 + exp(-(b2[c] + sum_j w2[c][j] hid[j])))
// all fp32, then  out = bf16(a + b + s * y * g[c])  on CC_PIX pixels, 8 channels per thread and step: one rounding.
constexpr int CC_PIX = 64, CC_SMAX = 64;
struct CombineArgs {
  const u16 *a, *b, *y; u16* out; long long lda, ldb, ldy, ldo, P;
  const float *mean, *w1, *b1, *w2, *b2;
  int C, Cs; float s;
};

__global__ void __launch_bounds__(256) channel_combine_kernel(const CombineArgs k) {
  __shared__ float s_hid[CC_SMAX];
  __shared__ float s_g[CM_CMAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* mean = k.mean + (long long)blockIdx.y * k.C;
  for (int j = wave; j < k.Cs; j += 4) {
    float s = 0.f;
    for (int c = lane; c < k.C; c += 64) s += k.w1[(long long)j * k.C + c] * mean[c];
    s = wave_sum(s) + k.b1[j];
    if (lane == 0) s_hid[j] = s > 0.f ? s : 0.f;
  }
  __syncthreads();
  for (int c = tid; c < k.C; c += 256) {
    float s = k.b2[c];
    for (int j = 0; j < k.Cs; ++j) s += k.w2[(long long)c * k.Cs + j] * s_hid[j];
    s_g[c] = 1.0f / (1.0f + expf(-s));
  }
  __syncthreads();
  const int C8 = k.C / 8;
  const long long p0 = (long long)blockIdx.x * CC_PIX, rest = k.P - p0;
  const int n = (int)(rest < CC_PIX ? rest : CC_PIX) * C8;
  const long long row0 = (long long)blockIdx.y * k.P + p0;
  for (int i = tid; i < n; i += 256) {
    const int p = i / C8, c = (i - p * C8) * 8;
    const long long row = row0 + p;
    float va[8], vb[8], vy[8], vo[8];
    unpack8(*(const uint4*)(k.a + row * k.lda + c), va);
    unpack8(*(const uint4*)(k.b + row * k.ldb + c), vb);
    unpack8(*(const uint4*)(k.y + row * k.ldy + c), vy);
#pragma unroll
    for (int j = 0; j < 8; ++j) vo[j] = va[j] + vb[j] + k.s * vy[j] * s_g[c + j];
    *(uint4*)(k.out + row * k.ldo + c) = pack8(vo);
  }
}

}  // namespace

int fluxmi_k_channel_mean(const void* x, long long ld, float* mean, float* work, long long work_bytes, int B, long long P, int C, hipStream_t s) {
  FLUXMI_REQUIRE(x && mean && work, "channel_mean: x, mean and work must not be NULL");
  FLUXMI_REQUIRE(C >= 8 && C <= CM_CMAX && C % 8 == 0, "channel_mean: C=%d must be a multiple of 8 in 8..%d", C, CM_CMAX);
  FLUXMI_REQUIRE(B >= 1 && B <= 65535 && P >= 1 && (P + CM_CHUNK - 1) / CM_CHUNK <= 2147483647LL,
                 "channel_mean: B=%d images / P=%lld pixels exceed the launch grid", B, P);
  FLUXMI_REQUIRE(ld % 8 == 0 && ld >= C, "channel_mean: the pixel stride ld=%lld must be a multiple of 8 and >= C = %d", ld, C);
  FLUXMI_REQUIRE((uintptr_t)x % 16 == 0 && ((uintptr_t)mean | (uintptr_t)work) % 4 == 0, "channel_mean: x must be 16-byte aligned (mean, work 4-byte)");
  const long long need = FLUXMI_CHANNEL_MEAN_WORK_BYTES(B, P, C);
  FLUXMI_REQUIRE(work_bytes >= need, "channel_mean: work must hold FLUXMI_CHANNEL_MEAN_WORK_BYTES(%d, %lld, %d) = %lld bytes (got %lld)", B, P, C,
                 need, work_bytes);
  const int nchunk = (int)((P + CM_CHUNK - 1) / CM_CHUNK);
  hipLaunchKernelGGL(channel_partial_kernel, dim3(nchunk, B), dim3(CM_THREADS), 0, s, (const u16*)x, ld, work, P, C, nchunk);
  FLUXMI_LAUNCH_CHECK();
  hipLaunchKernelGGL(channel_mean_kernel, dim3((C + CF_CH - 1) / CF_CH, B), dim3(CM_THREADS), 0, s, (const float*)work, mean, P, C, nchunk);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}

int fluxmi_k_channel_combine(const void* a, long long lda, const void* b, long long ldb, const void* y, long long ldy, const float* mean,
                             const float* w1, const float* b1, const float* w2, const float* b2, void* out, long long ldo, int B, long long P,
                             int C, int Cs, float scale, hipStream_t s) {
  FLUXMI_REQUIRE(a && b && y && mean && w1 && b1 && w2 && b2 && out, "channel_combine: no pointer may be NULL");
  FLUXMI_REQUIRE(C >= 8 && C <= CM_CMAX && C % 8 == 0, "channel_combine: C=%d must be a multiple of 8 in 8..%d", C, CM_CMAX);
  FLUXMI_REQUIRE(Cs >= 1 && Cs <= CC_SMAX, "channel_combine: the squeeze width Cs=%d must be in 1..%d", Cs, CC_SMAX);
  FLUXMI_REQUIRE(B >= 1 && B <= 65535 && P >= 1 && (P + CC_PIX - 1) / CC_PIX <= 2147483647LL,
                 "channel_combine: B=%d images / P=%lld pixels exceed the launch grid", B, P);
  FLUXMI_REQUIRE(lda % 8 == 0 && ldb % 8 == 0 && ldy % 8 == 0 && ldo % 8 == 0 && lda >= C && ldb >= C && ldy >= C && ldo >= C,
                 "channel_combine: every pixel stride must be a multiple of 8 and >= C = %d", C);
  FLUXMI_REQUIRE(((uintptr_t)a | (uintptr_t)b | (uintptr_t)y | (uintptr_t)out) % 16 == 0, "channel_combine: a, b, y and out must be 16-byte aligned");
  CombineArgs k;
  k.a = (const u16*)a; k.b = (const u16*)b; k.y = (const u16*)y; k.out = (u16*)out; k.lda = lda; k.ldb = ldb; k.ldy = ldy; k.ldo = ldo; k.P = P;
  k.mean = mean; k.w1 = w1; k.b1 = b1; k.w2 = w2; k.b2 = b2; k.C = C; k.Cs = Cs; k.s = scale;
  hipLaunchKernelGGL(channel_combine_kernel, dim3((unsigned)((P + CC_PIX - 1) / CC_PIX), B), dim3(256), 0, s, k);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}

int fluxmi_k_window_attention16(const void* qkv, long long ld, const float* table, int table_rows, const int* index, void* out, long long ldo,
                                int B, int H, int W, int heads, int shift, int overlap, float scale, hipStream_t s) {
  FLUXMI_REQUIRE(H >= WS && W >= WS && H % WS == 0 && W % WS == 0, "window_attention16: H=%d, W=%d must be positive multiples of the window %d", H, W, WS);
  FLUXMI_REQUIRE(overlap == 0 || overlap == OV, "window_attention16: overlap=%d must be 0 or %d", overlap, OV);
  FLUXMI_REQUIRE((shift == 0 || shift == WS / 2) && !(shift && overlap), "window_attention16: shift=%d must be 0 or %d, and 0 with an overlap", shift, WS / 2);
  FLUXMI_REQUIRE(heads >= 1 && heads <= 16, "window_attention16: heads=%d must be in 1..16", heads);
  FLUXMI_REQUIRE(table_rows >= 1 && table_rows <= TAB_MAX, "window_attention16: table_rows=%d must be in 1..%d (the head's column sits in LDS)", table_rows, TAB_MAX);
  const long long windows = (long long)(H / WS) * (W / WS);
  FLUXMI_REQUIRE(B >= 1 && B <= 65535 && windows <= 2147483647LL,
                 "window_attention16: B=%d images / %lld windows exceed the launch grid (65535 / 2^31 - 1)", B, windows);
  FLUXMI_REQUIRE(qkv && table && index && out, "window_attention16: qkv, table, index and out must not be NULL");
  const long long C = (long long)heads * HD;
  FLUXMI_REQUIRE(ld % 8 == 0 && ld >= 3 * C, "window_attention16: the qkv pixel stride ld=%lld must be a multiple of 8 and >= 3 * heads * 32 = %lld", ld, 3 * C);
  FLUXMI_REQUIRE(ldo % 8 == 0 && ldo >= C, "window_attention16: the out pixel stride ldo=%lld must be a multiple of 8 and >= heads * 32 = %lld", ldo, C);
  FLUXMI_REQUIRE(((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)index) % 16 == 0 && (uintptr_t)table % 4 == 0,
                 "window_attention16: qkv, out and index must be 16-byte aligned (table 4-byte)");
  const long long px = (long long)B * H * W;
  const uintptr_t q0 = (uintptr_t)qkv, q1 = q0 + (uintptr_t)(((px - 1) * ld + 3 * C) * 2);
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)(((px - 1) * ldo + C) * 2);
  FLUXMI_REQUIRE(o1 <= q0 || q1 <= o0, "window_attention16: out must not overlap qkv (a window's queries are other windows' keys)");
  Win16Args a;
  a.qkv = (const u16*)qkv; a.ld = ld; a.table = table; a.index = index; a.out = (u16*)out; a.ldo = ldo;
  a.H = H; a.W = W; a.heads = heads; a.shift = shift; a.overlap = overlap; a.table_rows = table_rows; a.scale = scale;
  // per device and cheap: set on every call, since the kernel cannot launch at all without it
  FLUXMI_CHECK_HIP(hipFuncSetAttribute((const void*)window_attention16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
  hipLaunchKernelGGL(window_attention16_kernel, dim3((unsigned)windows, B), dim3(WAVES * 64), (size_t)LDS_BYTES, s, a);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}
