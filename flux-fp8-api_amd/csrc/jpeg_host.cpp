// fluxmi -- the host half of the baseline JPEG encoder (include/fluxmi.h, fluxmi_jpeg_*): the plan of one encode -- geometry, the layout
// of the workspace, libjpeg's quality rule on the Annex K tables -- and the header bytes, SOI to SOS.  Plain C++; the kernels are jpeg.hip.
#include <string.h>

#include "fluxmi_internal.h"
#include "jpeg_tables.h"

using namespace fluxmi_jpeg;

namespace {

struct Writer {
  u8* p;
  int n;
  void byte(int v) { p[n++] = (u8)v; }
  void be16(int v) { byte(v >> 8); byte(v & 255); }
  void segment(int marker, int payload) { byte(0xFF); byte(marker); be16(payload + 2); }
};

void scaled_table(const u8* base, int quality, u8* zz) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int k = 0; k < 64; ++k) {
    int v = (base[kZigzag[k]] * s + 50) / 100;
    zz[k] = (u8)(v < 1 ? 1 : v > 255 ? 255 : v);
  }
}

void dht(Writer& w, int tc_th, const HuffSpec& t) {
  w.segment(0xC4, 1 + 16 + t.n);
  w.byte(tc_th);
  for (int i = 0; i < 16; ++i) w.byte(t.bits[i]);
  for (int i = 0; i < t.n; ++i) w.byte(t.vals[i]);
}

long long align_up(long long v, long long a) { return (v + a - 1) / a * a; }

}  // namespace

int fluxmi_jpeg_plan(const char* who, int B, int H, int W, int quality, int subsampling, int restart, FluxmiJpegPlan* p) {
  FLUXMI_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: B=%d, H=%d, W=%d must be >= 1", who, B, H, W);
  FLUXMI_REQUIRE(W <= 65535 && (long long)B * H <= 65535, "%s: a JPEG holds at most 65535 x 65535 pixels: W=%d, B * H = %d * %d = %lld rows", who,
                 W, B, H, (long long)B * H);
  FLUXMI_REQUIRE(quality >= 1 && quality <= 100, "%s: quality=%d must lie in 1..100", who, quality);
  FLUXMI_REQUIRE(subsampling == FLUXMI_JPEG_420 || subsampling == FLUXMI_JPEG_444, "%s: subsampling=%d must be FLUXMI_JPEG_420 (%d) or "
                 "FLUXMI_JPEG_444 (%d)", who, subsampling, FLUXMI_JPEG_420, FLUXMI_JPEG_444);
  FLUXMI_REQUIRE(restart >= 0 && restart <= 65535, "%s: restart=%d must lie in 0..65535 (MCUs per interval, 0 = none)", who, restart);
  memset(p, 0, sizeof(*p));
  const int m = subsampling == FLUXMI_JPEG_420 ? 16 : 8;
  p->H = H; p->Hs = B * H; p->W = W; p->ss = subsampling; p->bpm = subsampling == FLUXMI_JPEG_420 ? 6 : 3;
  p->mw = (W + m - 1) / m; p->mh = (p->Hs + m - 1) / m;
  p->nbw = (W + 7) / 8; p->nbh = (p->Hs + 7) / 8;
  p->n_mcu = (long long)p->mw * p->mh;
  p->R = restart > 0 && restart < p->n_mcu ? restart : (int)p->n_mcu;
  p->n_int = (p->n_mcu + p->R - 1) / p->R;
  p->stride = align_up((long long)p->R * p->bpm * kSlotBytesPerBlock + 16, 16);
  p->off_sizes = align_up(p->n_mcu * p->bpm * 64 * 2, 256);
  p->off_offs = align_up(p->off_sizes + p->n_int * 4, 256);
  p->off_slots = align_up(p->off_offs + p->n_int * 8, 256);
  p->work_bytes = p->off_slots + p->n_int * p->stride;
  scaled_table(kQLuma, quality, p->q[0]);
  scaled_table(kQChroma, quality, p->q[1]);

  Writer w{p->hdr, 0};
  w.byte(0xFF); w.byte(0xD8);
  w.segment(0xE0, 14);
  for (const char* c = "JFIF"; *c; ++c) w.byte(*c);
  w.byte(0); w.byte(1); w.byte(1); w.byte(0); w.be16(1); w.be16(1); w.byte(0); w.byte(0);
  for (int t = 0; t < 2; ++t) {
    w.segment(0xDB, 65);
    w.byte(t);
    for (int k = 0; k < 64; ++k) w.byte(p->q[t][k]);
  }
  w.segment(0xC0, 15);
  w.byte(8); w.be16(p->Hs); w.be16(W); w.byte(3);
  w.byte(1); w.byte(subsampling == FLUXMI_JPEG_420 ? 0x22 : 0x11); w.byte(0);
  w.byte(2); w.byte(0x11); w.byte(1);
  w.byte(3); w.byte(0x11); w.byte(1);
  dht(w, 0x00, kDcLuma);
  dht(w, 0x10, kAcLuma);
  dht(w, 0x01, kDcChroma);
  dht(w, 0x11, kAcChroma);
  if (restart > 0) {
    w.segment(0xDD, 2);
    w.be16(restart);
  }
  w.segment(0xDA, 10);
  w.byte(3); w.byte(1); w.byte(0x00); w.byte(2); w.byte(0x11); w.byte(3); w.byte(0x11); w.byte(0); w.byte(63); w.byte(0);
  p->hdr_bytes = w.n;
  // every interval: its slot's worst case + the RSTm or EOI behind it
  p->out_cap = p->hdr_bytes + p->n_mcu * p->bpm * kSlotBytesPerBlock + p->n_int * 4;
  return 0;
}

extern "C" {

int fluxmi_jpeg_workspace_bytes(int B, int H, int W, int subsampling, int restart, long long* work_bytes, long long* out_cap) {
  FluxmiJpegPlan p;
  FLUXMI_TRY(fluxmi_jpeg_plan("jpeg_workspace_bytes", B, H, W, 99, subsampling, restart, &p));
  if (work_bytes) *work_bytes = p.work_bytes;
  if (out_cap) *out_cap = p.out_cap;
  return 0;
}

int fluxmi_jpeg_header(int B, int H, int W, int quality, int subsampling, int restart, void* buf, long long cap, long long* n_bytes) {
  FluxmiJpegPlan p;
  FLUXMI_TRY(fluxmi_jpeg_plan("jpeg_header", B, H, W, quality, subsampling, restart, &p));
  FLUXMI_REQUIRE(buf && n_bytes, "jpeg_header: buf and n_bytes must not be NULL");
  FLUXMI_REQUIRE(cap >= p.hdr_bytes, "jpeg_header: buf holds %lld bytes, the header takes %d", cap, p.hdr_bytes);
  memcpy(buf, p.hdr, p.hdr_bytes);
  *n_bytes = p.hdr_bytes;
  return 0;
}

int fluxmi_jpeg_encode(const void* rgb, long long ld, long long bs, int B, int H, int W, int quality, int subsampling, int restart, void* work,
                       void* out, long long out_cap, void* n_bytes_dev, void* stream) {
  FluxmiJpegPlan p;
  FLUXMI_TRY(fluxmi_jpeg_plan("jpeg_encode", B, H, W, quality, subsampling, restart, &p));
  FLUXMI_REQUIRE(rgb, "jpeg_encode: rgb must not be NULL");
  FLUXMI_REQUIRE(ld >= 3LL * W, "jpeg_encode: rgb row stride %lld is shorter than its 3 W = %lld bytes", ld, 3LL * W);
  FLUXMI_REQUIRE(B == 1 || bs >= (long long)H * ld, "jpeg_encode: rgb image stride %lld is shorter than its H rows of %lld bytes", bs, ld);
  FLUXMI_REQUIRE(work && ((uintptr_t)work & 255) == 0, "jpeg_encode: work must be a 256-byte aligned device buffer of "
                 "fluxmi_jpeg_workspace_bytes' size (%lld bytes here)", p.work_bytes);
  FLUXMI_REQUIRE(out, "jpeg_encode: out must not be NULL");
  FLUXMI_REQUIRE(n_bytes_dev && ((uintptr_t)n_bytes_dev & 7) == 0, "jpeg_encode: n_bytes_dev must be an 8-byte aligned device address");
  FLUXMI_REQUIRE(out_cap >= p.hdr_bytes + 2, "jpeg_encode: out_cap=%lld is too small: the header and EOI alone take %d bytes (no stream "
                 "exceeds fluxmi_jpeg_workspace_bytes' out_cap = %lld)", out_cap, p.hdr_bytes + 2, p.out_cap);
  return fluxmi_k_jpeg_encode(p, rgb, ld, bs, work, out, out_cap, n_bytes_dev, (hipStream_t)stream);
}

int fluxmi_jpeg_finish(const void* n_bytes_dev, long long out_cap, long long* n_bytes, void* stream) {
  FLUXMI_REQUIRE(n_bytes_dev && n_bytes, "jpeg_finish: n_bytes_dev and n_bytes must not be NULL");
  long long n = 0;
  FLUXMI_CHECK_HIP(hipMemcpyAsync(&n, n_bytes_dev, sizeof(n), hipMemcpyDeviceToHost, (hipStream_t)stream));
  FLUXMI_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  *n_bytes = n;
  FLUXMI_REQUIRE(n <= out_cap, "jpeg_finish: out_cap=%lld is too small for a stream of %lld bytes: `out` holds its first out_cap bytes only", out_cap, n);
  return 0;
}

}  // extern "C"
