// fluxmi -- the baseline JPEG encoder's kernels (gfx950).  include/fluxmi.h (fluxmi_jpeg_*) states the arithmetic, jpeg_host.cpp plans an
// encode and writes the header; this file is the three stages, none of which waits on another workgroup:
//
// jpeg_transform_kernel   one workgroup = 16 x 16 pixels (one 4:2:0 MCU, or 2 x 2 4:4:4 MCUs).  A thread loads one pixel at an address clamped
//                         to the image (that clamp is the edge replication), converts it and stores the level-shifted samples block by block
//                         in LDS; 4:2:0 boxes the chroma there.  Eight threads per block run the row pass, then the column pass, of the integer
//                         DCT in place; all 256 quantise and store int16 levels in zigzag order, 128 bytes per block, MCU by MCU.
// jpeg_entropy_kernel     one workgroup (4 waves) = one restart interval, walked in chunks of 24 blocks, one wave per block and lane k on
//                         zigzag position k: a ballot is the block's non-zero mask, the distance to the previous set bit the lane's run; the
//                         lane forms its ZRL prefix and its (run, size) code + magnitude bits, a wave prefix sum places them, and they are OR-ed
//                         into a zeroed LDS bit buffer (LDS atomics: OR commutes, so the buffer does not depend on their order).  The chunk's
//                         whole bytes are then stuffed -- each thread a run of bytes, a workgroup prefix sum of their 0xFF counts -- and
//                         copied to the interval's slot; up to 7 bits carry into the next chunk.  The slot is written by this workgroup alone.
// jpeg_scan_kernel        one workgroup of 16 waves: the exclusive prefix sum of (interval bytes + 2 marker bytes) -> each interval's offset, and the total.
// jpeg_compact_kernel     copies every slot to its offset behind the header and appends RSTm (EOI behind the last); nothing at or beyond
//                         out + out_cap is written.  The header travels as kernel-argument data.
#include <string.h>

#include "common.h"
#include "fluxmi_internal.h"
#include "jpeg_tables.h"

namespace {

using namespace fluxmi_jpeg;

constexpr int CHUNK = 24;                       // blocks per chunk: FLUXMI_JPEG_RESTART_420 * 6 = FLUXMI_JPEG_RESTART_444 * 3
constexpr int WORDS_PER_BLOCK = 52;             // 1664 bits >= kMaxBlockBits
constexpr int BIT_WORDS = CHUNK * WORDS_PER_BLOCK + 2;   // + the carry of up to 7 bits
constexpr int OUT_BYTES = 2 * BIT_WORDS * 4;    // every byte 0xFF
static_assert(WORDS_PER_BLOCK * 32 >= kMaxBlockBits && CHUNK % 4 == 0, "chunk geometry");
static_assert(FLUXMI_JPEG_SLOT_BYTES_PER_BLOCK == kSlotBytesPerBlock, "header and tables disagree on the slot stride");

__device__ const HuffLut k_lut_dc[2] = {make_lut(kDcLuma), make_lut(kDcChroma)};
__device__ const HuffLut k_lut_ac[2] = {make_lut(kAcLuma), make_lut(kAcChroma)};

// ---- stage 1: colour, downsample, DCT, quantise ---------------------------------------------------------------------------------------------
struct TransformArgs {
  const u8* rgb;
  long long ld, bs;
  short* lev;
  int H, Hs, W, mw, mh, nbw, nbh, ss;
  u8 q[2][64];
};

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of the integer DCT over d[0], d[st], ..., d[7 st], in place
template <bool FIRST>
__device__ __forceinline__ void fdct8(int* d, int st) {
  constexpr int SH = FIRST ? 11 : 15;
  const int d0 = d[0], d1 = d[st], d2 = d[2 * st], d3 = d[3 * st], d4 = d[4 * st], d5 = d[5 * st], d6 = d[6 * st], d7 = d[7 * st];
  int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (FIRST) {
    d[0] = (t10 + t11) << 2;
    d[4 * st] = (t10 - t11) << 2;
  } else {
    d[0] = descale(t10 + t11, 2);
    d[4 * st] = descale(t10 - t11, 2);
  }
  int z1 = (t12 + t13) * 4433;
  d[2 * st] = descale(z1 + t13 * 6270, SH);
  d[6 * st] = descale(z1 - t12 * 15137, SH);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299;
  z1 *= -7373; z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7 * st] = descale(t4 + z1 + z3, SH);
  d[5 * st] = descale(t5 + z2 + z4, SH);
  d[3 * st] = descale(t6 + z2 + z3, SH);
  d[st] = descale(t7 + z1 + z4, SH);
}

__device__ __forceinline__ int quantise(int c, int t) { return c < 0 ? -((-c + 4 * t) / (8 * t)) : (c + 4 * t) / (8 * t); }

__global__ void __launch_bounds__(256) jpeg_transform_kernel(const TransformArgs a) {
  __shared__ int blk[12][64];      // 4:2:0: Y00 Y01 Y10 Y11 Cb Cr;  4:4:4: (Y Cb Cr) of the 2 x 2 MCUs, row-major
  __shared__ int chroma[2][256];   // 4:2:0: full-resolution Cb, Cr of the tile
  const int t = threadIdx.x, tx = blockIdx.x, ty = blockIdx.y;
  const bool s420 = a.ss == FLUXMI_JPEG_420;
  const int nblk = s420 ? 6 : 12;
  {
    const int py = t >> 4, px = t & 15;
    const int y = min(ty * 16 + py, a.Hs - 1), x = min(tx * 16 + px, a.W - 1);
    const int b = y / a.H, r = y - b * a.H;
    const u8* p = a.rgb + (long long)b * a.bs + (long long)r * a.ld + 3LL * x;
    const int R = p[0], G = p[1], B = p[2];
    const int Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
    const int Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
    const int Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
    const int quad = (py >> 3) * 2 + (px >> 3), e = (py & 7) * 8 + (px & 7);
    if (s420) {
      blk[quad][e] = Y - 128;
      chroma[0][t] = Cb;
      chroma[1][t] = Cr;
    } else {
      blk[quad * 3][e] = Y - 128;
      blk[quad * 3 + 1][e] = Cb - 128;
      blk[quad * 3 + 2][e] = Cr - 128;
    }
  }
  __syncthreads();
  if (s420 && t < 128) {
    const int c = t >> 6, cy = (t >> 3) & 7, cx = t & 7;
    // below the image the last chroma row repeats: chroma rows ceil(Hs / 2) of them, this tile starts at row 8 ty (which exists)
    const int lc = min(cy, (a.Hs + 1) / 2 - 1 - ty * 8);
    const int* s = &chroma[c][(2 * lc) * 16 + 2 * cx];
    blk[4 + c][cy * 8 + cx] = ((s[0] + s[1] + s[16] + s[17] + 1 + (cx & 1)) >> 2) - 128;
  }
  __syncthreads();
  if (t < nblk * 8) fdct8<true>(&blk[t >> 3][(t & 7) * 8], 1);
  __syncthreads();
  if (t < nblk * 8) fdct8<false>(&blk[t >> 3][t & 7], 8);
  __syncthreads();
  for (int e = t; e < nblk * 64; e += 256) {
    const int j = e >> 6, k = e & 63;
    if (s420) {
      int src = j;
      if (j >= 1 && j < 4) {  // dummy Y blocks: the DC level of the block before, no AC
        const bool right = tx * 2 + 1 >= a.nbw, below = ty * 2 + 1 >= a.nbh;
        const bool d1 = right, d2 = below, d3 = right || below;
        if (j == 1 && d1) src = 0;
        if (j == 2 && d2) src = d1 ? 0 : 1;
        if (j == 3 && d3) src = d2 ? (d1 ? 0 : 1) : 2;
      }
      int v;
      if (src != j) v = k == 0 ? quantise(blk[src][0], a.q[0][0]) : 0;
      else v = quantise(blk[j][kZigzag[k]], a.q[j >= 4][k]);
      a.lev[(((long long)ty * a.mw + tx) * 6 + j) * 64 + k] = (short)v;
    } else {
      const int quad = j / 3, c = j - quad * 3;
      const int my = ty * 2 + (quad >> 1), mx = tx * 2 + (quad & 1);
      if (my < a.mh && mx < a.mw) a.lev[(((long long)my * a.mw + mx) * 3 + c) * 64 + k] = (short)quantise(blk[j][kZigzag[k]], a.q[c > 0][k]);
    }
  }
}

// ---- stage 2: entropy coding ----------------------------------------------------------------------------------------------------------------
struct EntropyArgs {
  const short* lev;
  u8* slots;
  unsigned* sizes;
  long long stride, n_mcu;
  int R, bpm;
};

struct LaneCode {
  unsigned long long zbits;  // the ZRLs ahead of this lane's code: up to 3 x 11 bits
  unsigned cbits;            // Huffman code + magnitude bits: up to 26 bits
  int zlen, clen;
};

// v of `len` bits (len <= 33) into the big-endian bit buffer w at bit position p
__device__ __forceinline__ void put_bits(unsigned* w, int p, unsigned long long v, int len) {
  if (len == 0) return;
  const int s = p & 31, wi = p >> 5;
  const unsigned long long x = v << (64 - s - len);
  const unsigned hi = (unsigned)(x >> 32), lo = (unsigned)x;
  if (hi && wi < BIT_WORDS) atomicOr(&w[wi], hi);
  if (lo && wi + 1 < BIT_WORDS) atomicOr(&w[wi + 1], lo);
}

// the bits lane `lane` (zigzag position) contributes to the block at `lev`; pred = the DC level the difference is taken against
__device__ __forceinline__ LaneCode lane_code(const short* lev, int lane, int pred, int chroma, const unsigned* dc, const unsigned* ac) {
  const int v = lev[lane];
  const bool nz = lane > 0 && v != 0;
  const unsigned long long mask = __ballot(nz);
  LaneCode o = {0ull, 0u, 0, 0};
  dc += chroma * 16;
  ac += chroma * 256;
  if (lane == 0) {
    const int d = v - pred;
    const int n = min(32 - __clz(d < 0 ? -d : d), 11);
    const unsigned e = dc[n];
    o.cbits = ((e & 0xFFFFu) << n) | ((unsigned)(d < 0 ? d - 1 : d) & ((1u << n) - 1u));
    o.clen = (int)(e >> 16) + n;
  } else if (nz) {
    const unsigned long long below = mask & ((1ull << lane) - 1ull);
    const int prev = below ? 63 - __clzll((long long)below) : 0;
    const int run = lane - prev - 1;
    const unsigned z = ac[0xF0];
    for (int i = 0; i < (run >> 4); ++i) {
      o.zbits = (o.zbits << (z >> 16)) | (z & 0xFFFFu);
      o.zlen += (int)(z >> 16);
    }
    const int n = min(32 - __clz(v < 0 ? -v : v), 10);
    const unsigned e = ac[((run & 15) << 4) | n];
    o.cbits = ((e & 0xFFFFu) << n) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << n) - 1u));
    o.clen = (int)(e >> 16) + n;
  } else if (lane == 63) {  // level 63 is zero: end of block
    o.cbits = ac[0] & 0xFFFFu;
    o.clen = (int)(ac[0] >> 16);
  }
  return o;
}

// exclusive prefix sum of v over the 256 threads of the workgroup; *total = the sum.  scratch: 4 ints of LDS, reusable after the call
__device__ __forceinline__ int block_exclusive_scan(int v, int* scratch, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  __syncthreads();
  if (lane == 63) scratch[wave] = incl;
  __syncthreads();
  int base = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int s = scratch[w];
    if (w < wave) base += s;
    sum += s;
  }
  *total = sum;
  return base + incl - v;
}

__global__ void __launch_bounds__(256) jpeg_entropy_kernel(const EntropyArgs a) {
  __shared__ unsigned bits[BIT_WORDS];
  __shared__ u8 stuffed[OUT_BYTES];
  __shared__ unsigned lut_ac[512];
  __shared__ unsigned lut_dc[32];
  __shared__ int block_bits[CHUNK];
  __shared__ int scan_scratch[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  lut_ac[t] = k_lut_ac[0].v[t];
  lut_ac[256 + t] = k_lut_ac[1].v[t];
  if (t < 32) lut_dc[t] = (t & 15) < 12 ? k_lut_dc[t >> 4].v[t & 15] : 0u;

  const long long interval = blockIdx.x;
  const long long mcu0 = interval * a.R;
  const long long n_blocks = (min((long long)a.R, a.n_mcu - mcu0)) * a.bpm;  // of this interval
  const short* lev = a.lev + mcu0 * a.bpm * 64;
  u8* slot = a.slots + interval * a.stride;
  long long out_pos = 0;
  int carry_bits = 0;        // 0..7 bits of the previous chunk not yet written,
  unsigned carry_word = 0;   // left-aligned in a word
  for (long long b0 = 0; b0 < n_blocks; b0 += CHUNK) {
    const int n = (int)min((long long)CHUNK, n_blocks - b0);
    const bool last = b0 + CHUNK >= n_blocks;
    for (int i = t; i < BIT_WORDS; i += 256) bits[i] = 0u;
    __syncthreads();  // also: the tables are loaded
    LaneCode code[CHUNK / 4];
    int excl[CHUNK / 4];
#pragma unroll
    for (int i = 0; i < CHUNK / 4; ++i) {
      const int bi = i * 4 + wave;
      code[i] = LaneCode{0ull, 0u, 0, 0};
      excl[i] = 0;
      if (bi < n) {  // wave-uniform
        const long long g = b0 + bi;          // block of the interval
        const long long m = g / a.bpm;        // its MCU, counted from the interval's first
        const int j = (int)(g - m * a.bpm);
        const int chroma = a.bpm == 6 ? j >= 4 : j >= 1;
        long long prev = -1;                  // the previous block of the same component, within the interval
        if (a.bpm == 6 && j >= 1 && j < 4) prev = g - 1;
        else if (m > 0) prev = a.bpm == 6 && j == 0 ? g - 3 : g - a.bpm;
        const int pred = prev >= 0 ? (int)lev[prev * 64] : 0;
        code[i] = lane_code(lev + g * 64, lane, pred, chroma, lut_dc, lut_ac);
        int incl = code[i].zlen + code[i].clen;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const int up = __shfl_up(incl, d);
          if (lane >= d) incl += up;
        }
        excl[i] = incl - code[i].zlen - code[i].clen;
        if (lane == 63) block_bits[bi] = incl;
      }
    }
    __syncthreads();
    int total_bits = carry_bits;
#pragma unroll
    for (int i = 0; i < CHUNK / 4; ++i) {
      const int bi = i * 4 + wave;
      if (bi < n) {
        int base = carry_bits;
        for (int k = 0; k < bi; ++k) base += block_bits[k];
        put_bits(bits, base + excl[i], code[i].zbits, code[i].zlen);
        put_bits(bits, base + excl[i] + code[i].zlen, code[i].cbits, code[i].clen);
      }
    }
    for (int k = 0; k < n; ++k) total_bits += block_bits[k];
    if (t == 0 && carry_bits) atomicOr(&bits[0], carry_word);
    __syncthreads();
    // the chunk's whole bytes (the last chunk: every byte, padded with 1-bits), stuffed
    const int pad = last ? (8 - (total_bits & 7)) & 7 : 0;
    const int n_bytes = (total_bits + pad) >> 3;
    const int per = (n_bytes + 255) >> 8;
    const int j0 = min(t * per, n_bytes), j1 = min(j0 + per, n_bytes);
    int ff = 0;
    for (int j = j0; j < j1; ++j) {
      unsigned v = (bits[j >> 2] >> (24 - 8 * (j & 3))) & 255u;
      if (j == n_bytes - 1) v |= (1u << pad) - 1u;
      ff += v == 255u;
    }
    int ff_total;
    int o = j0 + block_exclusive_scan(ff, scan_scratch, &ff_total);
    for (int j = j0; j < j1; ++j) {
      unsigned v = (bits[j >> 2] >> (24 - 8 * (j & 3))) & 255u;
      if (j == n_bytes - 1) v |= (1u << pad) - 1u;
      stuffed[o++] = (u8)v;
      if (v == 255u) stuffed[o++] = 0;
    }
    // what is left of the bit buffer carries over
    carry_bits = (total_bits + pad) & 7;
    carry_word = carry_bits ? ((bits[n_bytes >> 2] >> (24 - 8 * (n_bytes & 3))) & 255u) << 24 : 0u;
    __syncthreads();
    const int n_out = n_bytes + ff_total;
    for (int j = t; j < n_out; j += 256)
      if (out_pos + j < a.stride) slot[out_pos + j] = stuffed[j];
    out_pos += n_out;
    __syncthreads();
  }
  if (t == 0) a.sizes[interval] = (unsigned)out_pos;
}

// ---- stage 3: offsets, then the file --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) jpeg_scan_kernel(const unsigned* sizes, unsigned long long* offs, long long n_int, int hdr_bytes,
                                                         unsigned long long* total) {
  __shared__ unsigned long long wave_sum[16];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long long per = (n_int + 1023) / 1024;  // consecutive intervals per thread
  const long long i0 = min(t * per, n_int), i1 = min(i0 + per, n_int);
  unsigned long long sum = 0;
  for (long long i = i0; i < i1; ++i) sum += sizes[i] + 2ull;  // + RSTm or EOI
  unsigned long long incl = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  unsigned long long run = (unsigned long long)hdr_bytes + incl - sum, all = hdr_bytes;
#pragma unroll
  for (int w = 0; w < 16; ++w) {
    const unsigned long long s = wave_sum[w];
    if (w < wave) run += s;
    all += s;
  }
  if (t == 0) *total = all;
  for (long long i = i0; i < i1; ++i) {
    offs[i] = run;
    run += sizes[i] + 2ull;
  }
}

struct CompactArgs {
  const u8* slots;
  const unsigned* sizes;
  const unsigned long long* offs;
  u8* out;
  long long stride, n_int, out_cap;
  int hdr_bytes;
  u8 hdr[640];
};

__global__ void __launch_bounds__(256) jpeg_compact_kernel(const CompactArgs a) {
  const long long i = blockIdx.x;
  const long long t = (long long)blockIdx.y * 256 + threadIdx.x, step = 256LL * gridDim.y;
  if (i == 0)
    for (long long j = t; j < a.hdr_bytes; j += step)
      if (j < a.out_cap) a.out[j] = a.hdr[j];
  const u8* src = a.slots + i * a.stride;
  const long long off = (long long)a.offs[i], n = min((long long)a.sizes[i], a.stride);
  for (long long j = t; j < n; j += step)
    if (off + j < a.out_cap) a.out[off + j] = src[j];
  if (t < 2 && off + n + t < a.out_cap) a.out[off + n + t] = t == 0 ? (u8)0xFF : (u8)(i == a.n_int - 1 ? 0xD9 : 0xD0 + (int)(i & 7));
}

}  // namespace

int fluxmi_k_jpeg_encode(const FluxmiJpegPlan& p, const void* rgb, long long ld, long long bs, void* work, void* out, long long out_cap,
                         void* n_bytes_dev, hipStream_t s) {
  u8* w = (u8*)work;
  short* lev = (short*)w;
  unsigned* sizes = (unsigned*)(w + p.off_sizes);
  unsigned long long* offs = (unsigned long long*)(w + p.off_offs);
  u8* slots = w + p.off_slots;
  FLUXMI_REQUIRE(p.n_int <= 0x7fffffffLL, "jpeg_encode: %lld restart intervals are beyond the launch grid", p.n_int);
  FLUXMI_REQUIRE(p.stride <= 0xffffffffLL, "jpeg_encode: an interval of %d MCUs may take %lld bytes, beyond the 32-bit interval sizes: use a "
                 "restart interval (restart = 0 codes the whole image as one)", p.R, p.stride);

  TransformArgs ta;
  ta.rgb = (const u8*)rgb; ta.ld = ld; ta.bs = bs; ta.lev = lev;
  ta.H = p.H; ta.Hs = p.Hs; ta.W = p.W; ta.mw = p.mw; ta.mh = p.mh; ta.nbw = p.nbw; ta.nbh = p.nbh; ta.ss = p.ss;
  memcpy(ta.q, p.q, sizeof(ta.q));
  hipLaunchKernelGGL(jpeg_transform_kernel, dim3((p.W + 15) / 16, (p.Hs + 15) / 16), dim3(256), 0, s, ta);
  FLUXMI_LAUNCH_CHECK();

  EntropyArgs ea;
  ea.lev = lev; ea.slots = slots; ea.sizes = sizes; ea.stride = p.stride; ea.n_mcu = p.n_mcu; ea.R = p.R; ea.bpm = p.bpm;
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)p.n_int), dim3(256), 0, s, ea);
  FLUXMI_LAUNCH_CHECK();

  hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(1024), 0, s, (const unsigned*)sizes, offs, p.n_int, p.hdr_bytes,
                     (unsigned long long*)n_bytes_dev);
  FLUXMI_LAUNCH_CHECK();

  CompactArgs ca;
  ca.slots = slots; ca.sizes = sizes; ca.offs = offs; ca.out = (u8*)out; ca.stride = p.stride; ca.n_int = p.n_int; ca.out_cap = out_cap;
  ca.hdr_bytes = p.hdr_bytes;
  memcpy(ca.hdr, p.hdr, sizeof(ca.hdr));
  const long long split = p.stride / 16384;
  hipLaunchKernelGGL(jpeg_compact_kernel, dim3((unsigned)p.n_int, (unsigned)(split < 1 ? 1 : split > 64 ? 64 : split)), dim3(256), 0, s, ca);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}
