// fluxmi -- the host half of the PNG encoder (include/fluxmi.h, fluxmi_png_*): the plan of one encode -- the strip rule, the slot size, the
// layout of the workspace -- the bytes in front of the deflate blocks, and the IDAT chunk's CRC-32 over the bytes the host has copied.
// Plain C++, nothing proportional to the pixel count but that CRC; the kernels are png.hip.
#include <string.h>

#include <chrono>

#include "fluxmi_internal.h"

namespace {

typedef unsigned char u8;
typedef unsigned int u32;

long long align_up(long long v, long long a) { return (v + a - 1) / a * a; }

void be32(u8* p, u32 v) {
  p[0] = (u8)(v >> 24); p[1] = (u8)(v >> 16); p[2] = (u8)(v >> 8); p[3] = (u8)v;
}

// CRC-32 (ISO 3309, the PNG specification's appendix), eight bytes a step
struct CrcTables {
  u32 t[8][256];
  CrcTables() {
    for (u32 i = 0; i < 256; ++i) {
      u32 c = i;
      for (int k = 0; k < 8; ++k) c = c & 1 ? 0xEDB88320u ^ (c >> 1) : c >> 1;
      t[0][i] = c;
    }
    for (u32 i = 0; i < 256; ++i)
      for (int k = 1; k < 8; ++k) t[k][i] = t[0][t[k - 1][i] & 255] ^ (t[k - 1][i] >> 8);
  }
};

u32 crc32(const u8* p, long long n) {
  static const CrcTables T;
  u32 c = 0xFFFFFFFFu;
  for (; n >= 8; n -= 8, p += 8) {
    const u32 lo = c ^ ((u32)p[0] | (u32)p[1] << 8 | (u32)p[2] << 16 | (u32)p[3] << 24);
    c = T.t[7][lo & 255] ^ T.t[6][(lo >> 8) & 255] ^ T.t[5][(lo >> 16) & 255] ^ T.t[4][lo >> 24] ^ T.t[3][p[4]] ^ T.t[2][p[5]] ^ T.t[1][p[6]] ^
        T.t[0][p[7]];
  }
  for (; n > 0; --n, ++p) c = T.t[0][(c ^ *p) & 255] ^ (c >> 8);
  return ~c;
}

}  // namespace

int fluxmi_png_plan(const char* who, int B, int H, int W, int C, int filter, FluxmiPngPlan* p) {
  FLUXMI_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: B=%d, H=%d, W=%d must be >= 1", who, B, H, W);
  FLUXMI_REQUIRE(C == 1 || C == 3, "%s: C=%d channels: a PNG of colour type 0 (grey, C = 1) or 2 (RGB, C = 3) is what is written", who, C);
  FLUXMI_REQUIRE(filter >= FLUXMI_PNG_FILTER_NONE && filter <= FLUXMI_PNG_FILTER_ADAPTIVE, "%s: filter=%d must be one of FLUXMI_PNG_FILTER_NONE "
                 "(0), _SUB, _UP, _AVERAGE, _PAETH, _ADAPTIVE (5)", who, filter);
  FLUXMI_REQUIRE((long long)B * H <= 0x7fffffffLL, "%s: B * H = %d * %d = %lld rows are beyond a PNG's 2^31 - 1", who, B, H,
                 (long long)B * H);
  FLUXMI_REQUIRE((long long)W * C < (1LL << 30), "%s: a row of W * C = %d * %d bytes is beyond the 2^30 a strip's 32-bit positions hold", who, W, C);
  memset(p, 0, sizeof(*p));
  p->H = H; p->Hs = B * H; p->W = W; p->C = C; p->filter = filter;
  p->row_bytes = 1 + W * C;
  const long long fit = FLUXMI_PNG_STRIP_TARGET / p->row_bytes;
  p->rows = (int)(fit < 1 ? 1 : fit > FLUXMI_PNG_STRIP_ROWS ? FLUXMI_PNG_STRIP_ROWS : fit);
  p->n_strips = ((long long)p->Hs + p->rows - 1) / p->rows;
  const long long strip_bytes = (long long)p->rows * p->row_bytes;
  FLUXMI_REQUIRE(p->n_strips * 256 <= 0xffffffffLL, "%s: %lld rows of %d bytes are %lld strips, beyond the %lld workgroups of 256 threads one "
                 "launch holds", who, (long long)p->Hs, p->row_bytes, p->n_strips, 0xffffffffLL / 256);
  p->in_lds = strip_bytes <= FLUXMI_PNG_STRIP_TARGET;
  p->lds_bytes = p->in_lds ? (int)align_up(strip_bytes, 16) : 0;
  p->res_stride = p->in_lds ? 0 : align_up(strip_bytes, 16);
  p->stride = align_up(FLUXMI_PNG_STRIP_BOUND(strip_bytes), 16);
  p->off_sizes = 0;
  p->off_offs = align_up(p->n_strips * 4, 256);
  p->off_adler = align_up(p->off_offs + p->n_strips * 8, 256);
  p->off_meta = align_up(p->off_adler + p->n_strips * 8, 256);
  p->off_slots = p->off_meta + 256;
  p->off_res = align_up(p->off_slots + p->n_strips * p->stride, 256);
  p->work_bytes = p->off_res + p->n_strips * p->res_stride;
  // every strip at its bound; the last strip may be shorter, which only lowers it
  const long long total = (long long)p->Hs * p->row_bytes;
  const long long tail_rows = p->Hs - (p->n_strips - 1) * p->rows;
  const long long payload = (p->n_strips - 1) * FLUXMI_PNG_STRIP_BOUND(strip_bytes) + FLUXMI_PNG_STRIP_BOUND(tail_rows * p->row_bytes) + 6;
  FLUXMI_REQUIRE(payload <= 0x7fffffffLL, "%s: %lld filtered bytes may take %lld bytes of one IDAT chunk, beyond its 2^31 - 1: several IDAT "
                 "chunks are not written", who, total, payload);
  p->out_cap = FLUXMI_PNG_HEAD_BYTES - 2 + payload + FLUXMI_PNG_TAIL_BYTES - 4;

  static const u8 sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  u8* h = p->head;
  memcpy(h, sig, 8);
  be32(h + 8, 13);
  memcpy(h + 12, "IHDR", 4);
  be32(h + 16, (u32)W);
  be32(h + 20, (u32)p->Hs);
  h[24] = 8; h[25] = C == 3 ? 2 : 0; h[26] = 0; h[27] = 0; h[28] = 0;
  be32(h + 29, crc32(h + 12, 17));
  be32(h + 33, 0);  // the IDAT payload's length: the scan kernel knows it
  memcpy(h + 37, "IDAT", 4);
  h[41] = 0x78; h[42] = 0x01;
  return 0;
}

extern "C" {

int fluxmi_png_workspace_bytes(int B, int H, int W, int C, long long* work_bytes, long long* out_cap) {
  FluxmiPngPlan p;
  FLUXMI_TRY(fluxmi_png_plan("png_workspace_bytes", B, H, W, C, FLUXMI_PNG_FILTER_ADAPTIVE, &p));
  if (work_bytes) *work_bytes = p.work_bytes;
  if (out_cap) *out_cap = p.out_cap;
  return 0;
}

int fluxmi_png_encode(const void* px, long long ld, long long bs, int B, int H, int W, int C, int filter, void* work, long long work_bytes,
                      void* out, long long out_cap, void* n_bytes_dev, void* stream) {
  FluxmiPngPlan p;
  FLUXMI_TRY(fluxmi_png_plan("png_encode", B, H, W, C, filter, &p));
  FLUXMI_REQUIRE(px, "png_encode: px must not be NULL");
  FLUXMI_REQUIRE(ld >= (long long)W * C, "png_encode: px row stride %lld is shorter than its W * C = %lld bytes", ld, (long long)W * C);
  FLUXMI_REQUIRE(B == 1 || bs >= (long long)H * ld, "png_encode: px image stride %lld is shorter than its H rows of %lld bytes", bs, ld);
  FLUXMI_REQUIRE(work && ((uintptr_t)work & 255) == 0, "png_encode: work must be a 256-byte aligned device buffer");
  FLUXMI_REQUIRE(work_bytes >= p.work_bytes, "png_encode: work holds %lld bytes, fluxmi_png_workspace_bytes gives %lld", work_bytes, p.work_bytes);
  FLUXMI_REQUIRE(out, "png_encode: out must not be NULL");
  FLUXMI_REQUIRE(n_bytes_dev && ((uintptr_t)n_bytes_dev & 7) == 0, "png_encode: n_bytes_dev must be an 8-byte aligned device address");
  FLUXMI_REQUIRE(out_cap >= FLUXMI_PNG_HEAD_BYTES + FLUXMI_PNG_TAIL_BYTES, "png_encode: out_cap=%lld is too small: the bytes around the deflate "
                 "blocks alone take %d (no file exceeds fluxmi_png_workspace_bytes' out_cap = %lld)", out_cap,
                 FLUXMI_PNG_HEAD_BYTES + FLUXMI_PNG_TAIL_BYTES, p.out_cap);
  return fluxmi_k_png_encode(p, px, ld, bs, work, out, out_cap, n_bytes_dev, (hipStream_t)stream);
}

int fluxmi_png_finish(const void* n_bytes_dev, long long out_cap, long long* n_bytes, void* stream) {
  FLUXMI_REQUIRE(n_bytes_dev && n_bytes, "png_finish: n_bytes_dev and n_bytes must not be NULL");
  long long n = 0;
  FLUXMI_CHECK_HIP(hipMemcpyAsync(&n, n_bytes_dev, sizeof(n), hipMemcpyDeviceToHost, (hipStream_t)stream));
  FLUXMI_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  *n_bytes = n;
  FLUXMI_REQUIRE(n <= out_cap, "png_finish: out_cap=%lld is too small for a file of %lld bytes: `out` holds its first out_cap bytes only", out_cap, n);
  return 0;
}

int fluxmi_png_header(int B, int H, int W, int C, void* buf, long long cap, long long* n_bytes) {
  FluxmiPngPlan p;
  FLUXMI_TRY(fluxmi_png_plan("png_header", B, H, W, C, FLUXMI_PNG_FILTER_ADAPTIVE, &p));
  FLUXMI_REQUIRE(buf && n_bytes, "png_header: buf and n_bytes must not be NULL");
  FLUXMI_REQUIRE(cap >= FLUXMI_PNG_HEAD_BYTES, "png_header: buf holds %lld bytes, the head takes %d", cap, FLUXMI_PNG_HEAD_BYTES);
  memcpy(buf, p.head, FLUXMI_PNG_HEAD_BYTES);
  *n_bytes = FLUXMI_PNG_HEAD_BYTES;
  return 0;
}

int fluxmi_png_seal(void* file, long long n_bytes, double* crc_ms) {
  u8* f = (u8*)file;
  FLUXMI_REQUIRE(f && n_bytes >= FLUXMI_PNG_HEAD_BYTES + FLUXMI_PNG_TAIL_BYTES, "png_seal: file must hold a whole file of fluxmi_png_encode "
                 "(%lld bytes given)", n_bytes);
  const long long payload = n_bytes - (FLUXMI_PNG_HEAD_BYTES - 2) - (FLUXMI_PNG_TAIL_BYTES - 4);
  FLUXMI_REQUIRE(memcmp(f + 37, "IDAT", 4) == 0 && payload == (long long)((u32)f[33] << 24 | (u32)f[34] << 16 | (u32)f[35] << 8 | (u32)f[36]),
                 "png_seal: the bytes are not a file of fluxmi_png_encode of %lld bytes (IDAT type or length)", n_bytes);
  const auto t0 = std::chrono::steady_clock::now();
  be32(f + 41 + payload, crc32(f + 37, 4 + payload));
  if (crc_ms) *crc_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

}  // extern "C"
