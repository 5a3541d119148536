// fluxmi -- adapter fuse into an e4m3 weight, in place and without an fp32 workspace (gfx950).
//
//   W' = requant( bf16( dequant(W) + sum_t d_t ) )        d_t: LoRA (chunk sum), LoHa, LoKr or a full delta   (include/fluxmi.h)
//
// One tiled kernel runs twice.  The MEASURE pass writes nothing to W: it rebuilds every element of its tile in registers and reduces
// max |bf16(.)| into amax_tmp[0] (atomic max on the bit pattern: the values are non-negative floats and a max has no order).  A one-lane
// kernel turns the amax into the new scale pair (amax_tmp[1 .. 2]; the old reciprocal is still needed), the WRITE pass recomputes the same
// tile with the same instructions and stores e4m3 bytes over the ones it read, and a last one-lane kernel publishes the scale pair.
// Recomputing a rank-r product costs 2 r flops per element on the matrix pipe; parking the element costs 8 bytes of HBM traffic.
//
// Work split.  A workgroup of eight waves owns a 128 x 128 tile of W; wave w owns rows [16 w, 16 w + 16) and all 128 columns as eight
// 16 x 16 MFMA blocks.  Block b holds the columns 8 c + b (c = 0 .. 15), NOT a contiguous eighth: a lane's eight blocks then hold eight
// neighbouring bytes of one row, so W is read and written 8 bytes per lane, 128 contiguous bytes per 16 lanes.  With K % 16 == 0 such a
// group is inside the matrix or outside it as a whole.
//
// Data movement.  Per rank chunk of 32 the factor panels of the tile are staged in LDS once and read by all waves, both as [r][128]:
//   rows panel (lora_B / w1_a / w2_a):  element (r, n) at r * 128 + (n ^ swz(r))   global reads run along r (contiguous); the xor spreads
//                                       the 64 lanes of a staging store, and the four ranks of an MFMA operand read, over the 64 banks
//   cols panel (lora_A / w1_b / w2_b):  element (r, k) at r * 128 + ((k % 8) ^ (r % 4)) * 16 + k / 8     block b's columns are contiguous
// so an MFMA operand is 16 consecutive floats per rank in four different bank groups (no conflict).  Rows and columns outside the matrix
// and ranks past the adapter's are staged as zeros.  v_mfma_f32_16x16x4_f32 keeps the factors in fp32 (a bf16 MFMA would round them); the
// sum runs in the instruction's fixed order, rank quads ascending.  LoHa keeps two accumulator sets and multiplies them in registers; a
// LoRA chunk sum uses the second set for the sum of the chunks.  LoKr and full deltas need no product: one gather each.
//
// Registers: 32 (tile) + 32 + 32 (accumulator sets) per lane, no scratch (profiles/adapter_fuse.txt has the compiler's figures).
//
// DoRA (fluxmi_adapter_fuse_dora_f8) is the same tile run three times with the term loop shared: see adapter_dora_kernel below.
#include "common.h"
#include "fluxmi_internal.h"

namespace {

constexpr int TILE = 128;  // rows and columns of W per workgroup
constexpr int RC = 32;     // ranks staged per LDS chunk
constexpr int PANEL = RC * TILE;

// the weight-scale rule of elementwise.hip (weight_scale_kernel; float8_quantize.py:198-203,214-215), restated here so that no step
// kernel's translation unit changes: reciprocal(amax) * max_val in two roundings, capped at max_val
__device__ __forceinline__ float recip_rn(float x) { return (float)(1.0 / (double)x); }
__global__ void adapter_scale_kernel(float* tmp) {
  const float s = fminf(recip_rn(fmaxf(tmp[0], 1e-12f)) * 448.0f, 448.0f);
  tmp[1] = s;
  tmp[2] = recip_rn(s);
}
__global__ void adapter_commit_kernel(const float* tmp, float* scale, float* recip) {
  *scale = tmp[1];
  *recip = tmp[2];
}
__global__ void adapter_clear_kernel(float* tmp) { tmp[0] = 0.f; }

constexpr int THREADS = 512;
// bank swizzle of the rows panel: ranks r .. r + 3 of an MFMA read land in four 16-bank groups, the 32 ranks of a staging store on 32 banks
__device__ __forceinline__ int swz(int r) { return ((r & 3) << 4) | (((r >> 2) & 7) << 1); }

// lora_B-like factor [N][R] -> rows panel.  Element e = tid + 512 i: rank e % 32 (contiguous in memory), tile row e / 32.
__device__ __forceinline__ void stage_rows(float* __restrict__ dst, const float* __restrict__ src, int R, int r0, int rlen, long long n0,
                                           int N, int tid) {
#pragma unroll 2
  for (int i = 0; i < PANEL / THREADS; ++i) {
    const int e = tid + THREADS * i, r = e & (RC - 1), n = e >> 5;
    const long long gn = n0 + n;
    dst[r * TILE + (n ^ swz(r))] = (r < rlen && gn < N) ? src[gn * R + r0 + r] : 0.f;
  }
}
// lora_A-like factor [R][K] -> cols panel.  Element e: tile column e % 128 (contiguous in memory), rank e / 128.
__device__ __forceinline__ void stage_cols(float* __restrict__ dst, const float* __restrict__ src, int K, int r0, int rlen, long long k0,
                                           int tid) {
#pragma unroll 2
  for (int i = 0; i < PANEL / THREADS; ++i) {
    const int e = tid + THREADS * i, kl = e & (TILE - 1), r = e >> 7;
    const long long gk = k0 + kl;
    dst[r * TILE + ((kl & 7) ^ (r & 3)) * 16 + (kl >> 3)] = (r < rlen && gk < K) ? src[(long long)(r0 + r) * K + gk] : 0.f;
  }
}
// P[b] += rows panel (this wave's 16 rows) x cols panel (block b's 16 columns) over `steps` rank quads; lane (c, h) feeds rank 4 s + h
__device__ __forceinline__ void panel_mfma(v4f (&P)[8], const float* __restrict__ rows, const float* __restrict__ cols, int steps, int wave,
                                           int c, int h) {
  for (int s = 0; s < steps; ++s) {
    const int r = 4 * s + h;
    const float a = rows[r * TILE + ((16 * wave + c) ^ swz(r))];
    const float* cp = cols + r * TILE + c;
#pragma unroll
    for (int b = 0; b < 8; ++b) P[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, cp[(b ^ h) * 16], P[b], 0, 0, 0);
  }
}

struct FuseArgs {
  fluxmi_delta_term_t t[FLUXMI_MAX_DELTA_TERMS];
  unsigned char* w;
  const float* recip;  // the reciprocal W was quantised with
  float* tmp;          // [0] amax, [1] new scale, [2] new reciprocal
  int n_terms, N, K, tiles_k;
};

// this lane's place in its tile: rows row0 + j (the C layout of the 16 x 16 MFMA), columns col + b
struct Lane {
  int tid, lane, wave, c, h;
  long long n0, k0, col, row0;
  bool ok[4];  // element (j, b) is inside the matrix
  __device__ __forceinline__ Lane(const FuseArgs& a) {
    tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, h = lane >> 4;
    n0 = (long long)(blockIdx.x / a.tiles_k) * TILE, k0 = (long long)(blockIdx.x % a.tiles_k) * TILE;
    col = k0 + 8 * c;
    row0 = n0 + 16 * wave + 4 * h;
#pragma unroll
    for (int j = 0; j < 4; ++j) ok[j] = col < a.K && row0 + j < a.N;
  }
};
// the eight dequantised weights of row j (zeros outside the matrix)
__device__ __forceinline__ void load_w(float (&w)[8], const FuseArgs& a, const Lane& L, int j, float recip) {
  const uint2 word = L.ok[j] ? *(const uint2*)(a.w + (L.row0 + j) * a.K + L.col) : make_uint2(0u, 0u);
#pragma unroll
  for (int b = 0; b < 8; ++b) w[b] = fp8_to_f32<FLUXMI_FMT_E4M3>(b < 4 ? word.x : word.y, b & 3) * recip;
}

// acc = fl(acc + d_t) in term order, for the tile's 32 elements of this lane
__device__ __forceinline__ void add_terms(v4f (&acc)[8], const FuseArgs& a, const Lane& L, float* lds) {
#pragma clang fp contract(off)  // a product and its scale are two roundings, never an fma with the add (include/fluxmi.h)
  const int tid = L.tid, wave = L.wave, c = L.c, h = L.h, N = a.N, K = a.K;
  const long long n0 = L.n0, k0 = L.k0, col = L.col, row0 = L.row0;
  const bool (&ok)[4] = L.ok;
  for (int t = 0; t < a.n_terms; ++t) {
    const fluxmi_delta_term_t T = a.t[t];
    if (T.kind == FLUXMI_DELTA_LORA || T.kind == FLUXMI_DELTA_LOHA) {
      const bool loha = T.kind == FLUXMI_DELTA_LOHA;
      const int chunks = loha ? 1 : T.n_chunks;
      v4f P[8], Q[8];  // LoRA: the current chunk's product and the sum of the chunks; LoHa: the two products
      // a chunk sum starts from +0 as fluxmi_lora_fuse_f8's does (a -0 delta becomes +0); a single chunk is taken as it is (-0 + x == x)
      const float q0 = loha || chunks > 1 ? 0.f : -0.f;
#pragma unroll
      for (int b = 0; b < 8; ++b) Q[b] = (v4f){q0, q0, q0, q0};
      for (int ch = 0; ch < chunks; ++ch) {
#pragma unroll
        for (int b = 0; b < 8; ++b) P[b] = (v4f){0.f, 0.f, 0.f, 0.f};
        const float* colsrc = T.p1 + (long long)ch * T.rank * K;
        for (int r0 = 0; r0 < T.rank; r0 += RC) {
          const int rlen = min(RC, T.rank - r0), steps = (rlen + 3) >> 2;
          __syncthreads();  // the previous chunk's panels have been read
          stage_rows(lds, T.p0, T.rank, r0, rlen, n0, N, tid);
          stage_cols(lds + PANEL, colsrc, K, r0, rlen, k0, tid);
          if (loha) {
            stage_rows(lds + 2 * PANEL, T.p2, T.rank, r0, rlen, n0, N, tid);
            stage_cols(lds + 3 * PANEL, T.p3, K, r0, rlen, k0, tid);
          }
          __syncthreads();
          panel_mfma(P, lds, lds + PANEL, steps, wave, c, h);
          if (loha) panel_mfma(Q, lds + 2 * PANEL, lds + 3 * PANEL, steps, wave, c, h);
        }
        if (!loha) {
#pragma unroll
          for (int b = 0; b < 8; ++b) Q[b] = Q[b] + P[b] * T.scale;
        }
      }
#pragma unroll
      for (int b = 0; b < 8; ++b) acc[b] = acc[b] + (loha ? (P[b] * Q[b]) * T.scale : Q[b]);
    } else if (T.kind == FLUXMI_DELTA_LOKR) {
      // torch.kron(w1, w2)[n][k] = w1[n / kn][k / kk] * w2[n % kn][k % kk]: the divisions are per row and per column, not per element
      const int w1_cols = K / T.kk;
      int i1[8], i2[8];
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const int k = col < K ? (int)col + b : 0;
        i1[b] = k / T.kk;
        i2[b] = k % T.kk;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (ok[j]) {
          const int n = (int)(row0 + j);  // < N: 32-bit divisions
          const float* p1 = T.p0 + (long long)(n / T.kn) * w1_cols;
          const float* p2 = T.p1 + (long long)(n % T.kn) * T.kk;
#pragma unroll
          for (int b = 0; b < 8; ++b) acc[b][j] = acc[b][j] + (p1[i1[b]] * p2[i2[b]]) * T.scale;
        }
      }
    } else {  // FLUXMI_DELTA_FULL
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (ok[j]) {
          const float* dp = T.p0 + (row0 + j) * K + col;
#pragma unroll
          for (int b = 0; b < 8; ++b) acc[b][j] = acc[b][j] + dp[b] * T.scale;
        }
      }
    }
  }
}

// eight bf16-valued floats of row j -> e4m3 bytes over the ones that were read: quantize_f32_kernel's expression (elementwise.hip)
__device__ __forceinline__ void store_row(const FuseArgs& a, const Lane& L, int j, const float (&o)[8], float scale) {
  float v[8];
#pragma unroll
  for (int b = 0; b < 8; ++b) v[b] = q_prepare<FLUXMI_FMT_E4M3>(o[b], scale);
  *(uint2*)(a.w + (L.row0 + j) * a.K + L.col) = make_uint2(cvt4_fp8<FLUXMI_FMT_E4M3>(v[0], v[1], v[2], v[3]), cvt4_fp8<FLUXMI_FMT_E4M3>(v[4], v[5], v[6], v[7]));
}
// the lanes' maxima -> amax_tmp[0]
__device__ __forceinline__ void tile_amax(float m, const FuseArgs& a, const Lane& L, float* lds) {
  m = wave_max(m);
  __syncthreads();  // the panels are dead: their first floats carry the waves' maxima
  if (L.lane == 0) lds[L.wave] = m;
  __syncthreads();
  if (L.tid == 0) {
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) m = fmaxf(m, lds[w]);
    if (m > 0.f) atomicMax((unsigned*)a.tmp, __float_as_uint(m));  // one atomic per workgroup
  }
}

template <bool WRITE>
__global__ void __launch_bounds__(THREADS) adapter_fuse_kernel(const FuseArgs a) {
#pragma clang fp contract(off)
  __shared__ float lds[4 * PANEL];
  const Lane L(a);
  v4f acc[8];
  {
    const float recip = *a.recip;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float w[8];
      load_w(w, a, L, j, recip);
#pragma unroll
      for (int b = 0; b < 8; ++b) acc[b][j] = w[b];
    }
  }
  add_terms(acc, a, L, lds);

  if (WRITE) {
    const float scale = a.tmp[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (L.ok[j]) {
        float o[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) o[b] = rbf(acc[b][j]);
        store_row(a, L, j, o, scale);
      }
    }
  } else {
    float m = 0.f;  // as amax_f32_as_bf16_kernel: fmaxf skips a NaN
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (L.ok[j]) {
#pragma unroll
        for (int b = 0; b < 8; ++b) m = fmaxf(m, fabsf(rbf(acc[b][j])));
      }
    }
    tile_amax(m, a, L, lds);
  }
}

// ---- DoRA: W' = requant(bf16(a_i * w + b_i * D)), (a_i, b_i) from the magnitude and the norm of w + D along one axis (include/fluxmi.h) ----
// Three tile passes.  NORM rebuilds v = w + D and leaves each tile's sums of squares in work; a one-lane-per-row kernel adds the tiles'
// partials in fp64, ascending, and writes the factor pair; MEASURE and WRITE recompute w and D and apply the pair.  REMOVE skips NORM and
// inverts the stored pair while it loads it.  D is built apart from w (the same add_terms on an accumulator that starts at -0: -0 + d == d for
// every d), and w is read again behind the terms, so the tile costs the registers it costs the additive kernel.
struct DoraArgs {
  const float* fac;  // [2][len]: a, b (MEASURE, WRITE)
  float* work;       // NORM: axis 0 [N][tiles_k], axis 1 [tiles_n][K]
  int len, remove;
};
enum { DORA_NORM = 0, DORA_MEASURE = 1, DORA_WRITE = 2 };

// the sum over the 16 lanes of a DPP row, left in all of them: lane ^ 8, ^ 4, ^ 2, ^ 1 (the controls of wave_butterfly, common.h)
__device__ __forceinline__ float row16_sum(float v) {
#pragma clang fp contract(off)
  auto dpp = [](float x, auto CTRL) {
    const int xi = __float_as_int(x);
    return __int_as_float(__builtin_amdgcn_update_dpp(xi, xi, decltype(CTRL)::value, 0xf, 0xf, false));
  };
  v = v + dpp(v, std::integral_constant<int, 0x128>{});  // row_ror:8
  v = v + dpp(v, std::integral_constant<int, 0x124>{});  // row_ror:4
  v = v + dpp(v, std::integral_constant<int, 0x4E>{});   // quad_perm:[2,3,0,1]
  v = v + dpp(v, std::integral_constant<int, 0xB1>{});   // quad_perm:[1,0,3,2]
  return v;
}
// fl(x / y): the quotient in fp64 rounds to the fp32 quotient (53 >= 2 * 24 + 2 bits), whatever division the compiler would pick
__device__ __forceinline__ float div_rn(float x, float y) { return (float)((double)x / (double)y); }

template <int PASS, int AXIS>
__global__ void __launch_bounds__(THREADS) adapter_dora_kernel(const FuseArgs a, const DoraArgs d) {
#pragma clang fp contract(off)  // two products and one add, each rounded
  __shared__ float lds[4 * PANEL];
  const Lane L(a);
  v4f D[8];
#pragma unroll
  for (int b = 0; b < 8; ++b) D[b] = (v4f){-0.f, -0.f, -0.f, -0.f};
  add_terms(D, a, L, lds);
  const float recip = *a.recip;

  if (PASS == DORA_NORM) {
    float ss[AXIS == 0 ? 4 : 8];  // axis 0: per row j over b ascending; axis 1: per column b over j ascending
#pragma unroll
    for (int i = 0; i < (AXIS == 0 ? 4 : 8); ++i) ss[i] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float w[8];
      load_w(w, a, L, j, recip);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const float v = L.ok[j] ? w[b] + D[b][j] : 0.f;  // outside the matrix: zeros
        ss[AXIS == 0 ? j : b] = ss[AXIS == 0 ? j : b] + v * v;
      }
    }
    if (AXIS == 0) {  // the 16 column lanes of a row are one DPP row; lane c == 0 (column k0, always inside) stores
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float s = row16_sum(ss[j]);
        if (L.c == 0 && L.row0 + j < a.N) d.work[(L.row0 + j) * a.tiles_k + blockIdx.x % a.tiles_k] = s;
      }
    } else {  // 32 row groups (wave, h) x 128 columns through LDS, summed by one lane per column in ascending row order
      __syncthreads();  // the panels are dead
#pragma unroll
      for (int b = 0; b < 8; ++b) lds[(4 * L.wave + L.h) * TILE + 8 * L.c + b] = ss[b];
      __syncthreads();
      if (L.tid < TILE) {
        float s = lds[L.tid];
        for (int g = 1; g < 32; ++g) s = s + lds[g * TILE + L.tid];
        if (L.k0 + L.tid < a.K) d.work[(long long)(blockIdx.x / a.tiles_k) * a.K + L.k0 + L.tid] = s;
      }
    }
    return;
  }

  float fa[AXIS == 0 ? 4 : 8], fb[AXIS == 0 ? 4 : 8];  // axis 0: one pair per lane-row; axis 1: one per lane-column
#pragma unroll
  for (int i = 0; i < (AXIS == 0 ? 4 : 8); ++i) {
    const long long idx = AXIS == 0 ? L.row0 + i : L.col + i;
    const bool in = AXIS == 0 ? L.row0 + i < a.N : L.col < a.K;
    fa[i] = in ? d.fac[idx] : 0.f;
    fb[i] = in ? d.fac[d.len + idx] : 0.f;
    if (d.remove) {  // a' = fl(1 / a), b' = -fl(b / a)
      fb[i] = -div_rn(fb[i], fa[i]);
      fa[i] = div_rn(1.f, fa[i]);
    }
  }
  const float scale = PASS == DORA_WRITE ? a.tmp[1] : 0.f;
  float m = 0.f;  // fmaxf skips a NaN
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (L.ok[j]) {
      float w[8], o[8];
      load_w(w, a, L, j, recip);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        o[b] = rbf(fa[AXIS == 0 ? j : b] * w[b] + fb[AXIS == 0 ? j : b] * D[b][j]);
        m = fmaxf(m, fabsf(o[b]));
      }
      if (PASS == DORA_WRITE) store_row(a, L, j, o, scale);
    }
  }
  if (PASS == DORA_MEASURE) tile_amax(m, a, L, lds);
}

// one lane per row (axis 0) or column (axis 1): the tiles' partials in fp64, ascending -> (a_i, b_i)
__global__ void dora_factors_kernel(const float* __restrict__ work, const float* __restrict__ mag, float* __restrict__ fac, int len, int tiles,
                                    long long stride_i, long long stride_t, float s) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= len) return;
  double ss = 0.0;
  for (int t = 0; t < tiles; ++t) ss = ss + (double)work[i * stride_i + t * stride_t];
  const float n = (float)sqrt(ss);
  const float b = s * div_rn(mag[i], n + 0x1p-23f);
  fac[i] = (1.f - s) + b;
  fac[len + i] = b;
}

FuseArgs fuse_args(void* w_fp8, float* w_scale_recip, const fluxmi_delta_term_t* terms, int n_terms, int N, int K, float* amax_tmp) {
  FuseArgs a;
  for (int t = 0; t < n_terms; ++t) a.t[t] = terms[t];
  for (int t = n_terms; t < FLUXMI_MAX_DELTA_TERMS; ++t) a.t[t] = fluxmi_delta_term_t{};
  a.w = (unsigned char*)w_fp8; a.recip = w_scale_recip; a.tmp = amax_tmp;
  a.n_terms = n_terms; a.N = N; a.K = K; a.tiles_k = (K + TILE - 1) / TILE;
  return a;
}

template <int AXIS>
void launch_dora(const FuseArgs& a, DoraArgs d, unsigned tiles, const float* magnitude, float strength, float* factors, float* w_scale,
                 float* w_scale_recip, hipStream_t s) {
  if (!d.remove) {
    const int tiles_n = (a.N + TILE - 1) / TILE;
    hipLaunchKernelGGL((adapter_dora_kernel<DORA_NORM, AXIS>), dim3(tiles), dim3(THREADS), 0, s, a, d);
    hipLaunchKernelGGL(dora_factors_kernel, dim3((d.len + 255) / 256), dim3(256), 0, s, (const float*)d.work, magnitude, factors, d.len,
                       AXIS == 0 ? a.tiles_k : tiles_n, (long long)(AXIS == 0 ? a.tiles_k : 1), (long long)(AXIS == 0 ? 1 : a.K), strength);
  }
  hipLaunchKernelGGL(adapter_clear_kernel, dim3(1), dim3(1), 0, s, a.tmp);
  hipLaunchKernelGGL((adapter_dora_kernel<DORA_MEASURE, AXIS>), dim3(tiles), dim3(THREADS), 0, s, a, d);
  hipLaunchKernelGGL(adapter_scale_kernel, dim3(1), dim3(1), 0, s, a.tmp);
  hipLaunchKernelGGL((adapter_dora_kernel<DORA_WRITE, AXIS>), dim3(tiles), dim3(THREADS), 0, s, a, d);
  hipLaunchKernelGGL(adapter_commit_kernel, dim3(1), dim3(1), 0, s, (const float*)a.tmp, w_scale, w_scale_recip);
}

}  // namespace

long long fluxmi_k_adapter_dora_work_bytes(int N, int K, int axis) {
  const long long tn = (N + TILE - 1) / TILE, tk = (K + TILE - 1) / TILE;
  return 4 * (axis == 0 ? (long long)N * tk : tn * K);
}

// everything validated by fluxmi_adapter_fuse_dora_f8 (api.cpp); factors: [2][N or K]; work: fluxmi_adapter_dora_work_bytes
int fluxmi_k_adapter_fuse_dora(void* w_fp8, float* w_scale, float* w_scale_recip, const fluxmi_delta_term_t* terms, int n_terms, int N, int K,
                               int axis, const float* magnitude, float strength, int remove, float* factors, float* work, float* amax_tmp,
                               hipStream_t s) {
  const FuseArgs a = fuse_args(w_fp8, w_scale_recip, terms, n_terms, N, K, amax_tmp);
  const long long tiles = (long long)((N + TILE - 1) / TILE) * a.tiles_k;
  FLUXMI_REQUIRE(tiles <= 0x7fffffffLL, "adapter_fuse_dora: %lld tiles exceed the grid", tiles);
  const DoraArgs d{factors, work, axis == 0 ? N : K, remove};
  if (axis == 0) launch_dora<0>(a, d, (unsigned)tiles, magnitude, strength, factors, w_scale, w_scale_recip, s);
  else launch_dora<1>(a, d, (unsigned)tiles, magnitude, strength, factors, w_scale, w_scale_recip, s);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}

// terms: validated by fluxmi_adapter_fuse_f8 (api.cpp); amax_tmp: four floats
int fluxmi_k_adapter_fuse(void* w_fp8, float* w_scale, float* w_scale_recip, const fluxmi_delta_term_t* terms, int n_terms, int N, int K,
                          float* amax_tmp, hipStream_t s) {
  const FuseArgs a = fuse_args(w_fp8, w_scale_recip, terms, n_terms, N, K, amax_tmp);
  const long long tiles = (long long)((N + TILE - 1) / TILE) * a.tiles_k;
  FLUXMI_REQUIRE(tiles <= 0x7fffffffLL, "adapter_fuse: %lld tiles exceed the grid", tiles);
  hipLaunchKernelGGL(adapter_clear_kernel, dim3(1), dim3(1), 0, s, amax_tmp);
  hipLaunchKernelGGL(adapter_fuse_kernel<false>, dim3((unsigned)tiles), dim3(THREADS), 0, s, a);
  hipLaunchKernelGGL(adapter_scale_kernel, dim3(1), dim3(1), 0, s, amax_tmp);
  hipLaunchKernelGGL(adapter_fuse_kernel<true>, dim3((unsigned)tiles), dim3(THREADS), 0, s, a);
  hipLaunchKernelGGL(adapter_commit_kernel, dim3(1), dim3(1), 0, s, (const float*)amax_tmp, w_scale, w_scale_recip);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}
