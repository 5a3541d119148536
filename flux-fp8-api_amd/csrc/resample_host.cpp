// fluxmi -- the host half of the image resampler (include/fluxmi.h, fluxmi_resample_*): Pillow's coefficient tables for one axis, in double
// with libm's sin / cos and in Pillow's operation order (another order can move a coefficient across its rounding step), and the plan of one
// resize -- which of the kernel's instantiations run (resample.hip).  Plain C++; needs no GPU.
#include <math.h>

#include "fluxmi_internal.h"

#pragma clang fp contract(off)  // no fused multiply-add may replace a rounded product below

namespace {

const double kPi = 3.14159265358979323846;

double sinc(double x) {
  if (x == 0.0) return 1.0;
  x = x * kPi;
  return sin(x) / x;
}
double f_box(double x) { return x > -0.5 && x <= 0.5 ? 1.0 : 0.0; }
double f_bilinear(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}
double f_hamming(double x) {
  if (x < 0.0) x = -x;
  if (x == 0.0) return 1.0;
  if (x >= 1.0) return 0.0;
  x = x * kPi;
  return sin(x) / x * (0.54f + 0.46f * cos(x));  // fp32 literals widened to double, as Pillow has them
}
double f_bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
double f_lanczos(double x) { return -3.0 <= x && x < 3.0 ? sinc(x) * sinc(x / 3) : 0.0; }

struct Filter {
  double (*f)(double);
  double support;
};
const Filter kFilters[5] = {{f_box, 0.5}, {f_bilinear, 1.0}, {f_hamming, 1.0}, {f_bicubic, 2.0}, {f_lanczos, 3.0}};

int axis_ok(const char* who, int n_in, int n_out, int filter) {
  FLUXMI_REQUIRE(filter >= 0 && filter < 5, "%s: filter=%d must be one of FLUXMI_RESAMPLE_BOX (0) .. FLUXMI_RESAMPLE_LANCZOS (4); NEAREST is a "
                 "different routine and is not provided", who, filter);
  FLUXMI_REQUIRE(n_in >= 1 && n_out >= 1 && n_in <= (1 << 24) && n_out <= (1 << 24), "%s: in=%d and out=%d must lie in 1..2^24", who, n_in, n_out);
  return 0;
}

}  // namespace

FluxmiResampleAxis fluxmi_resample_axis(int n_in, int n_out, int filter) {
  FluxmiResampleAxis a;
  a.n_in = n_in;
  a.scale = (double)n_in / n_out;
  const double fs = a.scale < 1.0 ? 1.0 : a.scale;
  a.support = kFilters[filter].support * fs;
  a.ss = 1.0 / fs;
  a.ksize = (int)ceil(a.support) * 2 + 1;
  return a;
}

void fluxmi_resample_bounds(const FluxmiResampleAxis& a, int xx, int* xmin, int* n) {
  const double center = (xx + 0.5) * a.scale;
  int lo = (int)(center - a.support + 0.5), hi = (int)(center + a.support + 0.5);
  if (lo < 0) lo = 0;
  if (hi > a.n_in) hi = a.n_in;
  *xmin = lo;
  *n = hi - lo;
}

extern "C" {

int fluxmi_resample_ksize(int n_in, int n_out, int filter, int* ksize) {
  FLUXMI_TRY(axis_ok("resample_ksize", n_in, n_out, filter));
  FLUXMI_REQUIRE(ksize, "resample_ksize: ksize must not be NULL");
  *ksize = fluxmi_resample_axis(n_in, n_out, filter).ksize;
  return 0;
}

int fluxmi_resample_coeffs(int n_in, int n_out, int filter, int* bounds, int* kk) {
  FLUXMI_TRY(axis_ok("resample_coeffs", n_in, n_out, filter));
  FLUXMI_REQUIRE(bounds && kk, "resample_coeffs: bounds [out][2] and kk [out][ksize] must not be NULL");
  const FluxmiResampleAxis a = fluxmi_resample_axis(n_in, n_out, filter);
  double (*const f)(double) = kFilters[filter].f;
  double* w = new double[a.ksize];
  for (int xx = 0; xx < n_out; ++xx) {
    const double center = (xx + 0.5) * a.scale;
    int xmin, n;
    fluxmi_resample_bounds(a, xx, &xmin, &n);
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
      w[x] = f((x + xmin - center + 0.5) * a.ss);
      ww += w[x];
    }
    int* k = kk + (long long)xx * a.ksize;
    for (int x = 0; x < a.ksize; ++x) {
      double v = x < n ? w[x] : 0.0;
      if (x < n && ww != 0.0) v /= ww;
      k[x] = v < 0 ? (int)(-0.5 + v * (1 << FLUXMI_RESAMPLE_PRECISION_BITS)) : (int)(0.5 + v * (1 << FLUXMI_RESAMPLE_PRECISION_BITS));
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = n;
  }
  delete[] w;
  return 0;
}

int fluxmi_resample_plan(int B, int H, int W, int C, int h, int w, int filter, int* fused, long long* work_bytes) {
  FluxmiResamplePlan p;
  FLUXMI_TRY(fluxmi_resample_make_plan("resample_plan", B, H, W, C, h, w, filter, &p));
  if (fused) *fused = p.fused;
  if (work_bytes) *work_bytes = p.work_bytes;
  return 0;
}

}  // extern "C"

// The plan.  A tile is FLUXMI_RESAMPLE_TILE_BYTES output bytes (pixels x channels) by FLUXMI_RESAMPLE_TILE_ROWS output rows.  Bounds are
// monotone in the output index, so a tile's footprint is [xmin(first), xmax(last)) x [ymin(first), ymax(last)).
int fluxmi_resample_make_plan(const char* who, int B, int H, int W, int C, int h, int w, int filter, FluxmiResamplePlan* p) {
  FLUXMI_REQUIRE(C == 1 || C == 3, "%s: C=%d must be 1 or 3 (Pillow premultiplies the alpha of a 4-channel image: not provided)", who, C);
  FLUXMI_REQUIRE(B >= 1 && B <= 65535, "%s: B=%d must lie in 1..65535", who, B);
  FLUXMI_TRY(axis_ok(who, W, w, filter));
  FLUXMI_TRY(axis_ok(who, H, h, filter));
  p->ax = fluxmi_resample_axis(W, w, filter);
  p->ay = fluxmi_resample_axis(H, h, filter);
  p->do_x = w != W;
  p->do_y = h != H;
  p->pitch = ((long long)w * C + 3) & ~3LL;
  int max_dw = 0, max_rows = 0;
  if (p->do_x) {
    for (long long e0 = 0; e0 < (long long)w * C; e0 += FLUXMI_RESAMPLE_TILE_BYTES) {
      long long e1 = e0 + FLUXMI_RESAMPLE_TILE_BYTES - 1;
      if (e1 > (long long)w * C - 1) e1 = (long long)w * C - 1;
      int x0, n0, x1, n1;
      fluxmi_resample_bounds(p->ax, (int)(e0 / C), &x0, &n0);
      fluxmi_resample_bounds(p->ax, (int)(e1 / C), &x1, &n1);
      const long long begin = ((long long)x0 * C) & ~3LL;
      const long long dw = ((long long)(x1 + n1) * C - begin + 3) >> 2;
      if (dw > max_dw) max_dw = dw > 0x7fffffff ? 0x7fffffff : (int)dw;
    }
  }
  if (p->do_y) {
    for (int y0 = 0; y0 < h; y0 += FLUXMI_RESAMPLE_TILE_ROWS) {
      const int y1 = y0 + FLUXMI_RESAMPLE_TILE_ROWS - 1 < h - 1 ? y0 + FLUXMI_RESAMPLE_TILE_ROWS - 1 : h - 1;
      int a0, n0, a1, n1;
      fluxmi_resample_bounds(p->ay, y0, &a0, &n0);
      fluxmi_resample_bounds(p->ay, y1, &a1, &n1);
      if (a1 + n1 - a0 > max_rows) max_rows = a1 + n1 - a0;
    }
  }
  FLUXMI_REQUIRE(max_dw <= FLUXMI_RESAMPLE_LDS_IN_BYTES / 4, "%s: the horizontal pass of %d -> %d columns needs %d bytes of one input row per "
                 "tile, more than its %d-byte stage (a horizontal reduction beyond about 60x -- with LANCZOS; the span is (tile pixels + 2 x "
                 "support) x the reduction -- is not provided)", who, W, w, 4 * max_dw, FLUXMI_RESAMPLE_LDS_IN_BYTES);
  p->fused = p->do_x && p->do_y && max_rows <= FLUXMI_RESAMPLE_LDS_MID_BYTES / FLUXMI_RESAMPLE_TILE_BYTES;
  p->work_bytes = p->do_x && p->do_y && !p->fused ? (long long)B * H * p->pitch : 0;
  return 0;
}
