// fluxmi -- the PNG encoder's kernels (gfx950).  include/fluxmi.h (fluxmi_png_*) states the format, png_host.cpp plans an encode and writes
// the bytes around the deflate blocks; this file is three launches, none of which waits on another workgroup:
//
// png_strip_kernel    one workgroup (4 waves) = one strip of whole rows = one deflate block.
//                     (1) filter: one wave per row; a lane walks the row 64 bytes apart, costs the five residual rows (sum of min(v, 256 - v),
//                         wave butterflies), and writes the chosen one behind its filter byte -- into LDS when the strip rule says a strip
//                         fits (FLUXMI_PNG_STRIP_TARGET), else into the strip's own range of `work` (a single row wider than that).
//                     (2) tokens: the strip is walked in chunks of 4096 bytes, 16 consecutive bytes (one 128-bit read) per thread.  A 16-bit
//                         mask says where runs start; a workgroup max-scan of each segment's last start gives every thread the start of the
//                         run it begins in, and a table of each segment's FIRST start (the chunk and 17 segments behind it) gives a match
//                         head its run's end within the 258 bytes it cares about.  That makes literal / match(length) / covered a closed
//                         form per byte.  Pass one counts symbols (LDS atomics) and sums the Adler-32 partial.
//                     (3) codes: a bitonic sort of the counts, one lane merges the two-queue Huffman tree and limits the lengths the way
//                         zlib does, canonical codes are bit-reversed into an LDS table; the same for the 19-symbol code of the header.
//                         Then the exact bit count decides between the dynamic block and stored blocks.
//                     (4) emit: pass two forms each thread's tokens again, a workgroup prefix sum places them, and they are OR-ed LSB first
//                         into a zeroed LDS window that is flushed to the strip's slot, up to 7 bits carried.  An empty stored block ends
//                         the strip on a byte.
// png_scan_kernel     one workgroup of 16 waves: the exclusive prefix sum of the strip sizes, the composition of the Adler-32 partials,
//                     the file's length.
// png_compact_kernel  copies every slot to its offset behind the head and writes head and tail; nothing at or beyond out + out_cap.
#include <limits.h>
#include <string.h>

#include "common.h"
#include "fluxmi_internal.h"

namespace {

typedef unsigned char u8;
typedef unsigned int u32;
typedef unsigned long long u64;

constexpr int NT = 256;
constexpr int SEG = 16;                 // bytes of one thread's segment
constexpr int CHUNK = NT * SEG;
constexpr int HALO = 17;                // segments behind a chunk that a head at its last byte may need: ceil((258 + 15) / 16)
constexpr int NSEG = NT + HALO;
constexpr int MAX_MATCH = 258;
constexpr int NSYM = 286, EOB = 256, NCL = 19;
constexpr int WIN_WORDS = (CHUNK * 15 + 21 + 18 + 7 + 31) / 32 + 2;  // a literal takes <= 15 bits; a head's 21 bits stand on >= 3 bytes
constexpr u32 ADLER = 65521u;
static_assert(WIN_WORDS * 32 >= 17 + 3 * NCL + 7 * (NSYM + 2) + 7, "the window holds the block header");
static_assert(FLUXMI_PNG_STRIP_TARGET % 16 == 0, "strips in LDS are read 16 bytes at a time");

struct StripArgs {
  const u8* px;
  long long ld, bs;
  u8* slots;
  u8* res;            // the filtered bytes of every strip when they do not live in LDS
  u32* sizes;
  u32* adler;         // per strip: sum of bytes, sum of (n - i) * byte, both mod 65521
  long long stride, res_stride, n_strips;
  int H, Hs, WC, C, row_bytes, rows, filter, in_lds;
};

// ---- workgroup scans over 256 threads (scratch: 4 ints of LDS, reusable after the call) -------------------------------------------------
template <class Op>
__device__ __forceinline__ int block_scan_exclusive(int v, int identity, Op op, int* scratch, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d);
    if (lane >= d) incl = op(incl, up);
  }
  int excl = __shfl_up(incl, 1);
  if (lane == 0) excl = identity;
  __syncthreads();
  if (lane == 63) scratch[wave] = incl;
  __syncthreads();
  int base = identity, all = identity;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int s = scratch[w];
    if (w < wave) base = op(base, s);
    all = op(all, s);
  }
  *total = all;
  return op(base, excl);
}
__device__ __forceinline__ int op_add(int a, int b) { return a + b; }
__device__ __forceinline__ int op_max(int a, int b) { return a > b ? a : b; }

// ---- the filters --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
  return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}
__device__ __forceinline__ int residual(int f, int x, int a, int b, int c) {
  const int pred = f == 0 ? 0 : f == 1 ? a : f == 2 ? b : f == 3 ? (a + b) >> 1 : paeth(a, b, c);
  return (x - pred) & 255;
}
__device__ __forceinline__ const u8* row_ptr(const StripArgs& a, long long y) {
  const long long b = y / a.H;
  return a.px + b * a.bs + (y - b * a.H) * a.ld;
}

// one wave filters row y of the stacked image into dst[0 .. row_bytes)
__device__ __forceinline__ void filter_row(const StripArgs& a, long long y, u8* dst) {
  const int lane = threadIdx.x & 63, C = a.C;
  const u8* cur = row_ptr(a, y);
  const u8* up = y > 0 ? row_ptr(a, y - 1) : nullptr;
  int f = a.filter;
  if (f == FLUXMI_PNG_FILTER_ADAPTIVE) {
    u64 cost[5] = {0, 0, 0, 0, 0};
    for (int i = lane; i < a.WC; i += 64) {
      const int x = cur[i], l = i >= C ? cur[i - C] : 0, u = up ? up[i] : 0, ul = up && i >= C ? up[i - C] : 0;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const int v = residual(k, x, l, u, ul);
        cost[k] += (u64)min(v, 256 - v);
      }
    }
    f = 0;
    u64 best = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      u64 c = cost[k];
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
      if (k == 0 || c < best) {  // ties keep the lower number
        best = c;
        f = k;
      }
    }
  }
  if (lane == 0) dst[0] = (u8)f;
  for (int i = lane; i < a.WC; i += 64) {
    const int x = cur[i], l = i >= C ? cur[i - C] : 0, u = up ? up[i] : 0, ul = up && i >= C ? up[i - C] : 0;
    dst[1 + i] = (u8)residual(f, x, l, u, ul);
  }
}

// ---- tokens -------------------------------------------------------------------------------------------------------------------------------
// the 16 bytes at res + p0 (p0 < n, a multiple of 16) and the mask of their run starts: bit j = byte p0 + j differs from the byte before it,
// is the strip's first byte, or lies at or beyond n
__device__ __forceinline__ u32 segment_starts(const u8* res, int p0, int n, uint4* bytes) {
  const uint4 v = *(const uint4*)(res + p0);
  *bytes = v;
  const u32 before = p0 > 0 ? res[p0 - 1] : 0u;
  const u32 d[4] = {v.x ^ ((v.x << 8) | before), v.y ^ ((v.y << 8) | (v.x >> 24)), v.z ^ ((v.z << 8) | (v.y >> 24)),
                    v.w ^ ((v.w << 8) | (v.z >> 24))};
  u32 mask = p0 == 0 ? 1u : 0u;
#pragma unroll
  for (int j = 0; j < SEG; ++j) mask |= ((d[j >> 2] >> (8 * (j & 3))) & 255u) ? 1u << j : 0u;
  if (n - p0 < SEG) mask |= (0xFFFFu << (n - p0)) & 0xFFFFu;
  return mask;
}

__device__ __forceinline__ int length_symbol(int len) {
  if (len == MAX_MATCH) return 285;
  const int l = len - 3;
  if (l < 8) return 257 + l;
  const int e = 29 - __clz(l);  // floor(log2 l) - 2
  return 261 + 4 * e + ((l >> e) & 3);
}
__device__ __forceinline__ int extra_bits(int sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }

// Front half of a chunk, the same in both passes: every thread's segment, the table of first starts, and the start of the run that the
// thread's first byte lies in.  Ends with the table visible to the workgroup.
struct Segment {
  uint4 bytes;
  u32 mask;
  int p0, run_start;
  bool live;
};
__device__ __forceinline__ Segment load_segment(const u8* res, int c0, int n, int* first_start, int* scratch, int* carry_start) {
  const int t = threadIdx.x;
  Segment s;
  s.p0 = c0 + t * SEG;
  s.live = s.p0 < n;
  s.mask = 0;
  s.bytes = make_uint4(0, 0, 0, 0);
  if (s.live) s.mask = segment_starts(res, s.p0, n, &s.bytes);
  first_start[t] = s.live ? (s.mask ? s.p0 + __ffs(s.mask) - 1 : INT_MAX) : n;
  if (t < HALO) {
    const int q0 = c0 + (NT + t) * SEG;
    int g = n;
    if (q0 < n) {
      uint4 dummy;
      const u32 m = segment_starts(res, q0, n, &dummy);
      g = m ? q0 + __ffs(m) - 1 : INT_MAX;
    }
    first_start[NT + t] = g;
  }
  const int last = s.mask ? s.p0 + 31 - __clz(s.mask) : -1;
  int total;
  const int before = block_scan_exclusive(last, -1, op_max, scratch, &total);
  s.run_start = max(before, *carry_start);
  *carry_start = max(total, *carry_start);
  return s;
}

// calls f(j, symbol, extra value) for the token that byte j of the segment starts (nothing for a covered byte)
template <class F>
__device__ __forceinline__ void walk_segment(const Segment& s, int n, const int* first_start, F&& f) {
  const int seg = threadIdx.x;
  const u32 w[4] = {s.bytes.x, s.bytes.y, s.bytes.z, s.bytes.w};
  int start = s.run_start;
#pragma unroll
  for (int j = 0; j < SEG; ++j) {
    const int p = s.p0 + j;
    if (p >= n) continue;
    const int byte = (int)((w[j >> 2] >> (8 * (j & 3))) & 255u);
    if ((s.mask >> j) & 1u) start = p;
    if (p == start) {
      f(j, byte, 0);
      continue;
    }
    const int r = (p - start - 1) % MAX_MATCH;  // the byte's place in its block of <= 258 copied bytes
    if (r >= 2) continue;
    // the run's end, as far as 258 bytes ahead matter
    int end = p + MAX_MATCH;
    const u32 rest = (s.mask >> j) >> 1;
    if (rest) {
      end = p + __ffs(rest);
    } else {
      for (int u = seg + 1; u <= seg + HALO; ++u) {
        const int g = first_start[u];
        if (g != INT_MAX) {
          end = g;
          break;
        }
      }
    }
    const int left = min(end - p, MAX_MATCH);  // equal bytes from p on
    if (r == 0) {
      if (left >= 3) {
        const int sym = length_symbol(left);
        f(j, sym, (left - 3) & ((1 << extra_bits(sym)) - 1));
      } else {
        f(j, byte, 0);
      }
    } else if (left < 2) {  // r == 1: the block began one byte back and is shorter than 3
      f(j, byte, 0);
    }
  }
}

// ---- Huffman code construction ------------------------------------------------------------------------------------------------------------
struct Build {
  u64 key[512];
  u32 weight[NSYM];        // of the internal nodes, in the order they were made
  unsigned short up_leaf[NSYM], up_node[NSYM];
  u8 depth[NSYM];
  int bl_count[16];
  u32 next[16];
};

// cnt[0 .. ntot) -> code[sym] = bit-reversed canonical code | length << 16 (0 for an unused symbol), lengths <= maxbits.  At least two
// symbols are in use.  The whole workgroup calls it.
__device__ void build_code(const u32* cnt, int ntot, int maxbits, u32* code, Build& b) {
  const int t = threadIdx.x;
  for (int i = t; i < 512; i += NT) b.key[i] = i < ntot && cnt[i] ? ((u64)cnt[i] << 16) | (u64)i : ~0ull;
  for (int i = t; i < ntot; i += NT) code[i] = 0u;
  __syncthreads();
  for (int k = 2; k <= 512; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), o = i | j;
      const u64 x = b.key[i], y = b.key[o];
      if ((x > y) == ((i & k) == 0)) {
        b.key[i] = y;
        b.key[o] = x;
      }
      __syncthreads();
    }
  if (t == 0) {
    int n = 0;
    while (n < ntot && b.key[n] != ~0ull) ++n;
    // two queues: the sorted leaves, and the internal nodes, whose weights come out in non-decreasing order
    int li = 0, ii = 0;
    for (int ni = 0; ni < n - 1; ++ni) {
      u32 wsum = 0;
      for (int k = 0; k < 2; ++k) {
        if (li < n && (ii >= ni || (u32)(b.key[li] >> 16) <= b.weight[ii])) {
          wsum += (u32)(b.key[li] >> 16);
          b.up_leaf[li++] = (unsigned short)ni;
        } else {
          wsum += b.weight[ii];
          b.up_node[ii++] = (unsigned short)ni;
        }
      }
      b.weight[ni] = wsum;
    }
    // depths from the root down, clamped; every clamped node counts, as in zlib's gen_bitlen
    for (int i = 0; i < 16; ++i) b.bl_count[i] = 0;
    int overflow = 0;
    b.depth[n - 2] = 0;
    for (int i = n - 3; i >= 0; --i) {
      int d = b.depth[b.up_node[i]] + 1;
      if (d > maxbits) d = maxbits, ++overflow;
      b.depth[i] = (u8)d;
    }
    for (int i = 0; i < n; ++i) {
      int d = b.depth[b.up_leaf[i]] + 1;
      if (d > maxbits) d = maxbits, ++overflow;
      ++b.bl_count[d];
    }
    while (overflow > 0) {
      int bits = maxbits - 1;
      while (b.bl_count[bits] == 0) --bits;
      --b.bl_count[bits];
      b.bl_count[bits + 1] += 2;
      --b.bl_count[maxbits];
      overflow -= 2;
    }
    // the rarest symbols take the longest codes
    int idx = 0;
    for (int bits = maxbits; bits >= 1; --bits)
      for (int c = b.bl_count[bits]; c > 0; --c) code[(int)(b.key[idx++] & 0xFFFFu)] = (u32)bits << 16;
    // canonical codes (RFC 1951 3.2.2), reversed: deflate packs a code from its most significant bit
    u32 c = 0;
    b.next[0] = 0;
    for (int bits = 1; bits <= maxbits; ++bits) {
      c = (c + (u32)b.bl_count[bits - 1]) << 1;
      b.next[bits] = c;
    }
    for (int s = 0; s < ntot; ++s) {
      const int len = (int)(code[s] >> 16);
      if (len) code[s] |= __brev(b.next[len]++) >> (32 - len);
    }
  }
  __syncthreads();
}

// ---- the bit window -----------------------------------------------------------------------------------------------------------------------
// a thread's consecutive tokens, OR-ed into the window a word at a time
struct BitSink {
  u32* win;
  u64 acc;
  int have, word;
  __device__ __forceinline__ BitSink(u32* w, int bitpos) : win(w), acc(0), have(bitpos & 31), word(bitpos >> 5) {}
  __device__ __forceinline__ void put(u32 bits, int n) {
    acc |= (u64)bits << have;
    have += n;
    if (have >= 32) {
      if (word < WIN_WORDS) atomicOr(&win[word], (u32)acc);
      ++word;
      acc >>= 32;
      have -= 32;
    }
  }
  __device__ __forceinline__ void done() {
    if ((u32)acc && word < WIN_WORDS) atomicOr(&win[word], (u32)acc);
  }
};

struct Flush {
  u8* slot;
  long long stride, pos;   // bytes written so far
  int carry_bits;          // 0 .. 7 bits not yet written,
  u32 carry;               // in the low bits
};
// the window holds fl.carry_bits + nbits bits (the carry not yet OR-ed in): its whole bytes go to the slot, the rest carries over.  Every
// put into the window has been issued before the call; on return the window is zero again.
__device__ __forceinline__ void flush_window(u32* win, int nbits, Flush& fl) {
  const int t = threadIdx.x;
  if (t == 0 && fl.carry_bits) atomicOr(&win[0], fl.carry);
  __syncthreads();
  const int total = fl.carry_bits + nbits, nbytes = total >> 3;
  for (int j = t; j < nbytes; j += NT)
    if (fl.pos + j < fl.stride) fl.slot[fl.pos + j] = (u8)(win[j >> 2] >> (8 * (j & 3)));
  fl.pos += nbytes;
  fl.carry_bits = total & 7;
  fl.carry = fl.carry_bits ? (win[nbytes >> 2] >> (8 * (nbytes & 3))) & ((1u << fl.carry_bits) - 1u) : 0u;
  __syncthreads();
  for (int j = t; j < (total + 31) / 32 && j < WIN_WORDS; j += NT) win[j] = 0u;
  __syncthreads();
}

__device__ const u8 k_cl_order[NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

extern __shared__ __attribute__((aligned(16))) unsigned char png_lds[];

__global__ void __launch_bounds__(NT) png_strip_kernel(const StripArgs a) {
  __shared__ union {
    Build build;
    u32 win[WIN_WORDS];
  } sh;
  __shared__ u32 hist[NSYM + 2], code[NSYM + 2], cl_cnt[NCL], cl_code[NCL];
  __shared__ int first_start[NSEG];
  __shared__ int scratch[4];
  __shared__ int hlit_s, hclen_s;
  const int t = threadIdx.x, wave = t >> 6;
  const long long strip = blockIdx.x;
  const long long y0 = strip * a.rows;
  const int rows = (int)min((long long)a.rows, a.Hs - y0);
  const int n = rows * a.row_bytes;
  u8* res = a.in_lds ? (u8*)png_lds : a.res + strip * a.res_stride;
  u8* slot = a.slots + strip * a.stride;

  // (1) filter
  for (int i = t; i < NSYM + 2; i += NT) hist[i] = 0u;
  if (t < NCL) cl_cnt[t] = 0u;
  for (int r = wave; r < rows; r += 4) filter_row(a, y0 + r, res + r * a.row_bytes);
  __syncthreads();

  // (2) pass one: symbol counts and the Adler-32 partial
  u64 sum_a = 0, sum_b = 0;
  int carry_start = 0;
  for (int c0 = 0; c0 < n; c0 += CHUNK) {
    const Segment s = load_segment(res, c0, n, first_start, scratch, &carry_start);
    if (s.live) {
      const u32 w[4] = {s.bytes.x, s.bytes.y, s.bytes.z, s.bytes.w};
#pragma unroll
      for (int j = 0; j < SEG; ++j)
        if (s.p0 + j < n) {
          const u32 v = (w[j >> 2] >> (8 * (j & 3))) & 255u;
          sum_a += v;
          sum_b += (u64)(n - s.p0 - j) * v;
        }
      walk_segment(s, n, first_start, [&](int, int sym, int) { atomicAdd(&hist[sym], 1u); });
    }
    __syncthreads();
  }
  if (t == 0) hist[EOB] = 1u;
  {
    int tot_a, tot_b;
    block_scan_exclusive((int)(sum_a % ADLER), 0, op_add, scratch, &tot_a);
    block_scan_exclusive((int)(sum_b % ADLER), 0, op_add, scratch, &tot_b);
    if (t == 0) {
      a.adler[2 * strip] = (u32)tot_a % ADLER;
      a.adler[2 * strip + 1] = (u32)tot_b % ADLER;
    }
  }
  __syncthreads();

  // (3) the two codes and the exact size of the dynamic block
  build_code(hist, NSYM, 15, code, sh.build);
  if (t == 0) hlit_s = EOB + 1;
  __syncthreads();
  for (int i = t; i < NSYM; i += NT)
    if (code[i]) atomicMax(&hlit_s, i + 1);
  __syncthreads();
  const int hlit = hlit_s;
  if (t == 0) code[hlit] = code[hlit + 1] = 1u << 16;  // the two distance codes, one bit each; read as lengths only
  __syncthreads();
  for (int i = t; i < hlit + 2; i += NT) atomicAdd(&cl_cnt[code[i] >> 16], 1u);
  __syncthreads();
  build_code(cl_cnt, NCL, 7, cl_code, sh.build);
  if (t == 0) {
    int h = NCL;
    while (h > 4 && (cl_code[k_cl_order[h - 1]] >> 16) == 0) --h;
    hclen_s = h;
  }
  __syncthreads();
  const int hclen = hclen_s;
  int matches = 0;
  u64 dyn_bits;
  {
    int mine = 0;  // a thread's share is below 2^31: the strip is at most 2^30 bytes of at most 21 bits, over 256 threads
    for (int i = t; i < hlit + 2; i += NT) mine += (int)(cl_code[code[i] >> 16] >> 16);
    u64 body = 0;
    for (int i = t; i < hlit; i += NT) {
      body += (u64)hist[i] * ((code[i] >> 16) + (u32)extra_bits(i));
      if (i > EOB) matches += (int)hist[i];
    }
    int hdr_total, m_total, lo_total, hi_total;
    block_scan_exclusive(mine, 0, op_add, scratch, &hdr_total);
    block_scan_exclusive(matches, 0, op_add, scratch, &m_total);
    block_scan_exclusive((int)(body & 0xFFFFFu), 0, op_add, scratch, &lo_total);
    block_scan_exclusive((int)(body >> 20), 0, op_add, scratch, &hi_total);
    dyn_bits = 17ull + 3ull * hclen + (u64)hdr_total + (u64)m_total + (u64)lo_total + ((u64)hi_total << 20);
  }
  const long long pieces = ((long long)n + 65534) / 65535;
  const u64 stored_bits = 8ull * (u64)n + 40ull * (u64)pieces;
  const u32 last = strip == a.n_strips - 1 ? 1u : 0u;
  long long out_bytes;

  if (dyn_bits >= stored_bits) {
    // stored blocks of at most 65535 bytes; the strip began on a byte
    for (long long k = t; k < pieces; k += NT) {
      const u32 len = (u32)min(65535LL, n - k * 65535);
      u8* h = slot + k * 65540;
      h[0] = 0;
      h[1] = (u8)len; h[2] = (u8)(len >> 8);
      h[3] = (u8)~len; h[4] = (u8)(~len >> 8);
    }
    for (int i = t; i < n; i += NT) slot[(long long)i + 5 * (i / 65535 + 1)] = res[i];
    out_bytes = (long long)n + 5 * pieces;
    if (t == 0) slot[out_bytes] = (u8)last;
    ++out_bytes;
  } else {
    // (4) the header, then pass two
    for (int i = t; i < WIN_WORDS; i += NT) sh.win[i] = 0u;
    __syncthreads();
    Flush fl = {slot, a.stride, 0, 0, 0u};
    {
      u32 bits[2];
      int len[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int i = t + k * NT;
        const u32 c = i < hlit + 2 ? cl_code[code[i] >> 16] : 0u;
        bits[k] = c & 0xFFFFu;
        len[k] = (int)(c >> 16);
      }
      // symbols t and t + 256 are not neighbours: place the first 256, then the rest behind them
      const int front = 17 + 3 * hclen;
      int total0, total1;
      const int at0 = block_scan_exclusive(len[0], 0, op_add, scratch, &total0);
      const int at1 = block_scan_exclusive(len[1], 0, op_add, scratch, &total1);
      if (t == 0) {
        BitSink sink(sh.win, 0);
        sink.put(0u | (2u << 1), 3);  // BFINAL 0, BTYPE 10
        sink.put((u32)(hlit - 257), 5);
        sink.put(1u, 5);              // HDIST: two codes
        sink.put((u32)(hclen - 4), 4);
        for (int i = 0; i < hclen; ++i) sink.put(cl_code[k_cl_order[i]] >> 16, 3);
        sink.done();
      }
      {
        BitSink sink(sh.win, front + at0);
        sink.put(bits[0], len[0]);
        sink.done();
      }
      {
        BitSink sink(sh.win, front + total0 + at1);
        sink.put(bits[1], len[1]);
        sink.done();
      }
      flush_window(sh.win, front + total0 + total1, fl);
    }
    // the distance codes are lengths no more: a match's distance bit rides on its length symbol
    carry_start = 0;
    for (int c0 = 0; c0 < n; c0 += CHUNK) {
      const Segment s = load_segment(res, c0, n, first_start, scratch, &carry_start);
      u32 tok[SEG];  // bits | count << 24
      int mine = 0;
#pragma unroll
      for (int j = 0; j < SEG; ++j) tok[j] = 0u;
      if (s.live)
        walk_segment(s, n, first_start, [&](int j, int sym, int extra) {
          const u32 c = code[sym];
          int len = (int)(c >> 16);
          u32 bits = c & 0xFFFFu;
          if (sym > EOB) {  // extra bits, then the distance code 0 of one bit
            bits |= (u32)extra << len;
            len += extra_bits(sym) + 1;
          }
          tok[j] = bits | (u32)len << 24;
          mine += len;
        });
      int total;
      const int at = block_scan_exclusive(mine, 0, op_add, scratch, &total);
      if (mine) {
        BitSink sink(sh.win, fl.carry_bits + at);
#pragma unroll
        for (int j = 0; j < SEG; ++j)
          if (tok[j]) sink.put(tok[j] & 0xFFFFFFu, (int)(tok[j] >> 24));
        sink.done();
      }
      if (c0 + CHUNK >= n) {  // end of block, then the empty stored block's three bits and the padding to a byte
        const int eob_len = (int)(code[EOB] >> 16);
        if (t == 0) {
          BitSink sink(sh.win, fl.carry_bits + total);
          sink.put(code[EOB] & 0xFFFFu, eob_len);
          sink.put(last, 3);
          sink.done();
        }
        total += eob_len + 3;
        total += (8 - ((fl.carry_bits + total) & 7)) & 7;
      }
      flush_window(sh.win, total, fl);
    }
    out_bytes = fl.pos;
  }
  // LEN = 0, NLEN = 0xFFFF of the empty stored block
  if (t < 4 && out_bytes + t < a.stride) slot[out_bytes + t] = t < 2 ? (u8)0 : (u8)0xFF;
  if (t == 0) a.sizes[strip] = (u32)(out_bytes + 4);
}

// ---- offsets, checksum, file --------------------------------------------------------------------------------------------------------------
struct AdlerPart {
  u32 a, b, n;  // all mod 65521
};
__device__ __forceinline__ AdlerPart adler_join(const AdlerPart& x, const AdlerPart& y) {
  return AdlerPart{(x.a + y.a) % ADLER, (u32)((x.b + (u64)y.n * x.a + y.b) % ADLER), (x.n + y.n) % ADLER};
}

struct ScanArgs {
  const u32* sizes;
  const u32* adler;
  u64* offs;
  u32* meta;        // [0] the Adler-32, [1] the IDAT payload's length
  u64* total;
  long long n_strips;
  int Hs, rows, row_bytes;
};

__global__ void __launch_bounds__(1024) png_scan_kernel(const ScanArgs a) {
  __shared__ u64 wave_sum[16];
  __shared__ AdlerPart part[1024];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long long per = (a.n_strips + 1023) / 1024;  // consecutive strips per thread
  const long long i0 = min(t * per, a.n_strips), i1 = min(i0 + per, a.n_strips);
  u64 sum = 0;
  AdlerPart mine = {0u, 0u, 0u};
  for (long long i = i0; i < i1; ++i) {
    sum += a.sizes[i];
    const long long rows = min((long long)a.rows, a.Hs - i * a.rows);
    mine = adler_join(mine, AdlerPart{a.adler[2 * i], a.adler[2 * i + 1], (u32)((u64)rows * a.row_bytes % ADLER)});
  }
  part[t] = mine;
  u64 incl = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  u64 run = (u64)FLUXMI_PNG_HEAD_BYTES + incl - sum, all = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) {
    const u64 s = wave_sum[w];
    if (w < wave) run += s;
    all += s;
  }
  for (long long i = i0; i < i1; ++i) {
    a.offs[i] = run;
    run += a.sizes[i];
  }
  if (t == 0) {
    AdlerPart all_parts = {0u, 0u, 0u};
    for (int k = 0; k < 1024; ++k) all_parts = adler_join(all_parts, part[k]);
    // the stream starts from (1, 0): a = 1 + sum, b = n + weighted sum
    a.meta[0] = ((all_parts.b + all_parts.n) % ADLER) << 16 | (1u + all_parts.a) % ADLER;
    a.meta[1] = (u32)(all + 6);  // zlib header 2, Adler-32 4
    *a.total = all + FLUXMI_PNG_HEAD_BYTES + FLUXMI_PNG_TAIL_BYTES;
  }
}

struct CompactArgs {
  const u8* slots;
  const u32* sizes;
  const u64* offs;
  const u32* meta;
  u8* out;
  long long stride, n_strips, out_cap;
  u8 head[FLUXMI_PNG_HEAD_BYTES];
};

__global__ void __launch_bounds__(256) png_compact_kernel(const CompactArgs a) {
  const long long i = blockIdx.x;
  const long long t = (long long)blockIdx.y * 256 + threadIdx.x, step = 256LL * gridDim.y;
  if (i == 0 && t < FLUXMI_PNG_HEAD_BYTES && t < a.out_cap) {
    const u32 idat = a.meta[1];
    a.out[t] = t >= 33 && t < 37 ? (u8)(idat >> (8 * (36 - t))) : a.head[t];
  }
  const u8* src = a.slots + i * a.stride;
  const long long off = (long long)a.offs[i], n = min((long long)a.sizes[i], a.stride);
  for (long long j = t; j < n; j += step)
    if (off + j < a.out_cap) a.out[off + j] = src[j];
  if (i == a.n_strips - 1 && t < FLUXMI_PNG_TAIL_BYTES && off + n + t < a.out_cap) {
    // the Adler-32, the IDAT's CRC (left zero: the host fills it in over the bytes it copies), IEND
    const u8 iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    const u32 adler = a.meta[0];
    a.out[off + n + t] = t < 4 ? (u8)(adler >> (8 * (3 - t))) : t < 8 ? (u8)0 : iend[t - 8];
  }
}

}  // namespace

int fluxmi_k_png_encode(const FluxmiPngPlan& p, const void* px, long long ld, long long bs, void* work, void* out, long long out_cap,
                        void* n_bytes_dev, hipStream_t s) {
  u8* w = (u8*)work;
  u32* sizes = (u32*)(w + p.off_sizes);
  u64* offs = (u64*)(w + p.off_offs);
  u32* adler = (u32*)(w + p.off_adler);
  u32* meta = (u32*)(w + p.off_meta);
  u8* slots = w + p.off_slots;

  StripArgs sa;
  sa.px = (const u8*)px; sa.ld = ld; sa.bs = bs; sa.slots = slots; sa.res = w + p.off_res; sa.sizes = sizes; sa.adler = adler;
  sa.stride = p.stride; sa.res_stride = p.res_stride; sa.n_strips = p.n_strips;
  sa.H = p.H; sa.Hs = p.Hs; sa.WC = p.W * p.C; sa.C = p.C; sa.row_bytes = p.row_bytes; sa.rows = p.rows; sa.filter = p.filter; sa.in_lds = p.in_lds;
  FLUXMI_CHECK_HIP(hipFuncSetAttribute((const void*)png_strip_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, FLUXMI_PNG_STRIP_TARGET));
  hipLaunchKernelGGL(png_strip_kernel, dim3((unsigned)p.n_strips), dim3(NT), (size_t)p.lds_bytes, s, sa);
  FLUXMI_LAUNCH_CHECK();

  ScanArgs sc;
  sc.sizes = sizes; sc.adler = adler; sc.offs = offs; sc.meta = meta; sc.total = (u64*)n_bytes_dev; sc.n_strips = p.n_strips;
  sc.Hs = p.Hs; sc.rows = p.rows; sc.row_bytes = p.row_bytes;
  hipLaunchKernelGGL(png_scan_kernel, dim3(1), dim3(1024), 0, s, sc);
  FLUXMI_LAUNCH_CHECK();

  CompactArgs ca;
  ca.slots = slots; ca.sizes = sizes; ca.offs = offs; ca.meta = meta; ca.out = (u8*)out; ca.stride = p.stride; ca.n_strips = p.n_strips;
  ca.out_cap = out_cap;
  memcpy(ca.head, p.head, sizeof(ca.head));
  const long long split = p.stride / 16384;
  hipLaunchKernelGGL(png_compact_kernel, dim3((unsigned)p.n_strips, (unsigned)(split < 1 ? 1 : split > 64 ? 64 : split)), dim3(256), 0, s, ca);
  FLUXMI_LAUNCH_CHECK();
  return 0;
}
