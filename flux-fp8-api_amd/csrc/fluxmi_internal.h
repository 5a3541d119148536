// fluxmi -- internal launch descriptors shared by the kernels, the C-ABI layer and the engine.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/fluxmi.h"

typedef fluxmi_gemm_group_t FluxmiGemmGroup;

// ---- weight prefetch riding on another launch -------------------------------------------------------------------------------------
// Inside the denoise step every F8Linear weight is read ONCE per step: 11.9 GB stream through the 256 MB Infinity Cache, so a GEMM's
// first tiles find their W panels in HBM and run their K loops ~20 % longer than the later tiles, whose panels another XCD has
// already pulled on chip (profiles/r04_gemm_persist.txt: in-step timeline 78 K -> 60 K cycles per tile; the back-to-back probe never
// shows it).  Launches that leave CUs idle -- attention's 432 workgroups = 1.69 rounds of the 256 CUs, the 216-tile GEMMs -- therefore
// carry a few EXTRA workgroups behind their own that do nothing but read the weights of the launches that follow (16 B per lane,
// results discarded): the lines land in the memory-side cache, where every XCD finds them.  Purely a hint: no output depends on it.
struct FluxmiPrefetch {
  const void* ptr[6];
  long long bytes[6];  // multiples of 16
  int n;               // ranges in use
  int wgs;             // extra workgroups the launch appends for it (0 = off)
};
// engine -> next launch that supports it (attention, the 256x256 one-tile-per-workgroup GEMMs); consumed by that launch.  Thread-local.
void fluxmi_set_prefetch(const FluxmiPrefetch* pf);
FluxmiPrefetch fluxmi_take_prefetch();

#define FLUXMI_MAX_GROUPS 16
struct FluxmiGemmParams {
  FluxmiGemmGroup g[FLUXMI_MAX_GROUPS];
  int n_groups, N, K, epi, tiles_m_total, group_m;
  // split-K (small-M launches, gemm_pp.hip): `split_k` workgroups per tile, each over its own K range, fp32 partial tiles in
  // partial[split][tiles_m_total * 256][N]; fluxmi_launch_splitk_reduce sums them in split order and applies the epilogue
  int split_k;
  float* partial;
  unsigned long long* dbg;  // per-tile timestamps of the persistent kernel's timing build (tile config 19), else null
  FluxmiPrefetch pf;        // weights of later launches, read by pf.wgs extra workgroups behind the tiles (see FluxmiPrefetch)
  // implicit 3x3 convolution (round 6, fluxmi_conv3x3 -> the 128x128 tile kernel only; C == 0: off): the A operand is never materialised --
  // row r of group 0 is output pixel (b, yo, xo) of a [B, Ho, Wo] grid and K index (tap, c) reads x[b, (yo*stride + dy - pad) >> rshift,
  // (xo*stride + dx - pad) >> rshift, c] of the NHWC input g[0].A (zero outside [0, Hi << rshift)): what fluxmi_im2col3x3 would have written
  struct { const void* zeros; int Hi, Wi, C, Ho, Wo, stride, pad, rshift; } conv;
};

// ---- batched skinny GEMV (modulations + embedders, M = batch <= 8) ----------------------------
struct FluxmiGemvLayer {
  const void* W;           // [N,K] fp8 or bf16
  const void* bias;        // bf16 [N] or nullptr
  const float* in_scale;   // fp8: device scalar input_scale
  const float* sa_recip;   // fp8
  const float* sb_recip;   // fp8
  void* out;               // bf16, row b at out + b*ld_out
  const void* x;           // bf16 [B,K] (row stride ldx)
  long long ld_out, ldx;
  int N, K;
  int w_fp8;               // 1: fp8 weights (x quantised on the fly), 0: bf16 weights
  int pre_silu;            // apply SiLU (rounded to bf16) to x first        flux_model.py:252,155,496
  int blk_start;           // first block id of this layer (filled by launcher)
  int act_fmt;
};

struct FluxmiCalibLayer { float* trials; float* scale; float* recip; };

// ---- misc ------------------------------------------------------------------------------------
void fluxmi_set_error(const char* fmt, ...);
#define FLUXMI_CHECK_HIP(expr)                                                            \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess) {                                                               \
      fluxmi_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return 2;                                                                           \
    }                                                                                     \
  } while (0)
#define FLUXMI_REQUIRE(cond, ...)            \
  do {                                       \
    if (!(cond)) {                           \
      fluxmi_set_error(__VA_ARGS__);         \
      return 1;                              \
    }                                        \
  } while (0)
#define FLUXMI_LAUNCH_CHECK() FLUXMI_CHECK_HIP(hipGetLastError())
#define FLUXMI_TRY(expr)        \
  do {                          \
    int _rc = (expr);           \
    if (_rc) return _rc;        \
  } while (0)

// ---- kernel-selection knobs (tuning.cpp): a copy of the process-wide struct, and the counter fluxmi_set_tuning bumps
fluxmi_tuning_t fluxmi_tuning();
unsigned fluxmi_tuning_generation();
void fluxmi_log_tuning(const char* why);

// ---- internal launchers (defined in the .hip files) --------------------------------------------
int fluxmi_gemm_tile_ok(int N, int K, int is_fp8, int cfg);  // gemm_dispatch.cpp: config cfg of the table (gemm_cfg.h) tiles this shape
int fluxmi_launch_gemm(FluxmiGemmParams& p, int is_fp8, int act_fmt, int tile_cfg, hipStream_t s);  // gemm.hip: validates, then the family's launcher:
int fluxmi_launch_gemm_pp(FluxmiGemmParams& p, int is_fp8, int act_fmt, hipStream_t s);           // ping-pong ring (gemm_pp.hip)
int fluxmi_launch_gemm_w1(FluxmiGemmParams& p, int is_fp8, int act_fmt, int cfg, hipStream_t s);  // one wave per SIMD, every height (gemm_w1.hip)
int fluxmi_launch_gemm_generic(FluxmiGemmParams& p, int is_fp8, int act_fmt, hipStream_t s);
const void* fluxmi_zero_page();  // 256 zero bytes on the current device (vae.hip; allocated once per device, never under stream capture)
int fluxmi_launch_gemm_conv(FluxmiGemmParams& p, hipStream_t s);  // bf16, tile config 2 with the implicit 3x3 gather (p.conv filled by the caller)
// persistent 256x256 ping-pong kernel (gemm_persist.hip, tile config 18; 19 = with per-tile timestamps)
int fluxmi_gemm_persist_ok(const FluxmiGemmParams& p, int is_fp8, int act_fmt);
int fluxmi_launch_gemm_persist(FluxmiGemmParams& p, int is_fp8, int act_fmt, int timing, hipStream_t s);
// 256x256 ping-pong tiles with `split_k` K ranges per tile + the reduce / epilogue pass (BF16 and GATE_RESID epilogues)
void fluxmi_gemm_block_splitk(int on);  // +1 / -1: no M-dependent split-K choice while > 0 (thread-local)
int fluxmi_launch_gemm_splitk(FluxmiGemmParams& p, int is_fp8, int act_fmt, int split_k, hipStream_t s);
// split-K partial-tile scratch of the calling thread's launches (thread-local; nullptr = the library's own per-(device, stream) buffer, which is
// allocated at the first EAGER use on that stream and refuses to appear under stream capture).  An engine owns one and sets it around its launches:
// its step graph is captured on a private stream and replayed on the caller's, so the scratch must belong to the engine, not to a stream.
constexpr size_t FLUXMI_SPLITK_WS_BYTES = (size_t)256 << 20;
void fluxmi_set_splitk_scratch(float* p);
// the batch of the calling thread's engine (1 = none): bf16 launches take the split-K decision of ONE sample's groups, so a sample's bits do not
// follow the batch it rides in (gemm_dispatch.cpp)
void fluxmi_gemm_set_batch(int B);
// scratch of attention's balanced grid (attention2.hip, AttnSplit: partial softmax states of the key bins + arrival counters, which must be
// ZERO when handed over and are left zero by every launch): thread-local like the split-K scratch, an engine owns one; nullptr = the library's own
// per-(device, stream) buffer.  fluxmi_attn_plan_any: does a balanced-grid plan exist for one sample of this shape (any tuning)?
constexpr size_t FLUXMI_ATTN_SPLIT_WS_BYTES = (size_t)8 * 64 * (8 * 17 * 64 * 4) * 4 + 8 * 64 * 4;
void fluxmi_set_attn_scratch(void* p);
int fluxmi_attn_plan_any(int B, int L, int H);
int fluxmi_attn_debug_buffer(void* dev_u64);  // fluxmi_attention_debug_buffer
int fluxmi_attn_plan_export(int B, int L, int H, int* n_per_x, int* full_per_x, int* npieces, unsigned long long* pieces);  // fluxmi_attention_plan  // the same for ANY tuning (what an engine sizes its workspace by: the knob may change later)
// gemm_dispatch.cpp: plan the launches of a grouped GEMM of any number of groups (tile choice, peel, split-K, chunks of FLUXMI_MAX_GROUPS), then
// issue them; fluxmi_gemm_plan_export = the plan alone (fluxmi_gemm_plan)
int fluxmi_gemm_dispatch(const FluxmiGemmGroup* gs, int n, int N, int K, int is_fp8, int act_fmt, int epi, hipStream_t s);
int fluxmi_gemm_plan_export(const FluxmiGemmGroup* gs, int n, int N, int K, int is_fp8, int act_fmt, int epi, int batch, int* plan, int plan_cap,
                            int* plan_len);
int fluxmi_launch_gemv(const FluxmiGemvLayer* layers_dev, FluxmiGemvLayer* layers_host, int n_layers, int B, int total_blocks,
                       int max_K, hipStream_t s, int row0 = 0);
int fluxmi_gemv_blocks(const FluxmiGemvLayer* layers_host, int n_layers);

int fluxmi_k_quantize_act(const void* x, void* q, const float* scale, int rows, int cols, long long ld_in, long long ld_out, int fmt, hipStream_t s);
int fluxmi_k_amax(const void* x, float* amax, int rows, int cols, long long ld, hipStream_t s);
int fluxmi_k_calib_update(const float* amax, float* trials, float* scale, float* recip, int trial_index, int num_trials, float max_val, hipStream_t s);
int fluxmi_k_calib_update_many(const float* amax, const void* layers_dev, int n_layers, int trial_index, int num_trials, float max_val, hipStream_t s);
int fluxmi_k_quantize_weight(const void* w_bf16, void* q, float* amax_tmp, float* scale, float* recip, int N, int K, int fmt, hipStream_t s);
int fluxmi_k_dequant(const void* q, float* out, const float* recip, long long n, int fmt, hipStream_t s);
int fluxmi_k_requantize_f32(const float* w32, void* q, float* amax_tmp, float* scale, float* recip, long long n, int fmt, hipStream_t s);
int fluxmi_k_lora_delta(const float* Bm, const float* A, float* delta, int N, int K, int R, float scale, int accumulate, hipStream_t s);
int fluxmi_k_axpy_f32(float* w, const float* d, float alpha, long long n, hipStream_t s);
int fluxmi_ln_pairs_ok(int H);  // elementwise.hip: fluxmi_k_ln_modulate can write the row-pair layout at this hidden size / ln_variant
int fluxmi_k_ln_modulate(const void* x, long long ldx, long long x_bstride, void* out, long long ldo, long long out_bstride,
                         const void* shift0, const void* scale0, const void* shift1, const void* scale1, long long mod_bstride,
                         const float* q0, const float* q1, int B, int L, int split, int H, int out_fp8, int fmt, hipStream_t s, int out_pairs = 0);
int fluxmi_k_act(const void* x, void* y, int rows, int cols, long long ld_in, long long ld_out, int mode, hipStream_t s);
int fluxmi_k_gate_residual(const void* x, const void* y, const void* gate, void* out, int B, int L, int H, long long ldx,
                           long long ldy, long long ldo, long long gate_bstride, hipStream_t s);
int fluxmi_k_add(const void* a, const void* b, void* z, long long n, hipStream_t s);
int fluxmi_k_build_qlut(const float* scale, int fmt, int act, void* lut, hipStream_t s);
int fluxmi_k_pair_rows(const void* in, void* out, int rows, long long row_bytes, hipStream_t s);
int fluxmi_k_unpair_rows(const void* in, void* out, int rows, long long row_bytes, hipStream_t s);  // the inverse
int fluxmi_k_add_bcast(const void* a, const void* b, void* z, long long rows, int nb, int cols, hipStream_t s);
int fluxmi_k_select_step(const void* table, const int* step, const int* step0_dev, void* dst, long long bytes, hipStream_t s);
int fluxmi_k_timestep_rows(void* t_rows, const float* ts, int step0, int B, int R, hipStream_t s);
int fluxmi_k_fill_bf16(void* dst, float v, int n, hipStream_t s);
int fluxmi_k_timestep_embedding(const void* t, const float* freqs, void* out, int B, int half, float time_factor, hipStream_t s);
int fluxmi_k_rope_table(const void* ids, const float* omega, const int* axis, void* pe, long long rows, int n_axes, int pairs, hipStream_t s);
// The update kernels (update_step.hip).  The flat Euler step img [n] += bf16(dts[*step] * pred [n]), any n % 8 == 0
int fluxmi_k_euler(void* img, const void* pred, const float* dts, const int* step, long long n, hipStream_t s);
// ... and every Euler step of a shaped stream, ONE kernel: the leading pred_rows rows of each sample (FLUX.1 Kontext: the reference rows
// stay) and the leading c_out channels of every row (Fill / Depth / Canny: the conditioning channels stay) of img [B, img_rows, c_in] +=
// bf16(dts[*step] * v), v = pred [B, pred_rows, c_out].  scale != NULL is the guided step and x0 != NULL appends the inpainting blend, both as
// below; `who` names the caller in a refusal.  The two entries below are this one behind their own NULL-argument checks
int fluxmi_k_euler_step(const char* who, void* img, const void* pred, const void* x0, const void* noise, const void* mask, const float* dts,
                        const float* tnext, const float* one_minus_tnext, const float* thr, const int* step, const float* scale, int B,
                        long long img_rows, long long pred_rows, int c_in, int c_out, hipStream_t s);
// the guided Euler step (true CFG): img [2B, img_rows, c_in], pred [2B, pred_rows, c_out], prompt branch first; both halves of img get
// x + bf16(dt * (u + s (c - u))) with one bf16 rounding per operation, s = *scale (device), dt = dts[*step]
int fluxmi_k_cfg_euler(void* img, const void* pred, const float* dts, const int* step, const float* scale, int B, long long img_rows,
                       long long pred_rows, int c_in, int c_out, hipStream_t s);
// the masked-latent update: the Euler step (scale != NULL: the guided one, img / pred [2B, ...]) then the blend with x0 re-noised to the next
// time; x0 / noise / mask dense bf16 [B, pred_rows, c_out], tnext / one_minus_tnext / thr fp32 tables indexed by *step like dts; thr != NULL
// replaces mask by (float(mask) > thr[*step])
int fluxmi_k_blend_euler(void* img, const void* pred, const void* x0, const void* noise, const void* mask, const float* dts, const float* tnext,
                         const float* one_minus_tnext, const float* thr, const int* step, const float* scale, int B, long long img_rows,
                         long long pred_rows, int c_in, int c_out, hipStream_t s);
// the table-driven solver update (fluxmi.h, fluxmi_solver_step): row *step of coef [n][8] / ctl [n][4] decides the linear update of x from
// x, the saved iterate xs, g = ga x + gb v and the two fp32 history slots; x0 != NULL appends blend_euler's blend, scale != NULL is the guided form
int fluxmi_k_solver_step(void* img, const void* pred, void* xs, float* hist, const float* coef, const int* ctl, const void* x0, const void* noise,
                         const void* mask, const float* tnext, const float* one_minus_tnext, const float* thr, const int* step,
                         const float* scale, int B, long long img_rows, long long pred_rows, int c_in, int c_out, hipStream_t s);
// ... with the stochastic samplers' last term acc + cn * z (fluxmi.h, fluxmi_solver_step_noise): cn = column 7 of the row, z the Philox
// normals of (ids[image], *step + *eval_offset, element); and the generator alone (fluxmi_philox_normal)
int fluxmi_k_solver_step_noise(void* img, const void* pred, void* xs, float* hist, const float* coef, const int* ctl, const void* x0,
                               const void* noise, const void* mask, const float* tnext, const float* one_minus_tnext, const float* thr,
                               const int* step, const float* scale, int B, long long img_rows, long long pred_rows, int c_in, int c_out,
                               const unsigned* ids, const int* eval_offset, hipStream_t s);
int fluxmi_k_philox_normal(void* out, const unsigned* ids, int B, long long n_per_image, unsigned eval, int raw, hipStream_t s);
// FlowEdit (flowedit.hip; include/fluxmi.h, fluxmi_flowedit_couple / _step): the coupling alone at host scalars (t, 1 - t, eval), and the update
// of the edit state z from row *step of coef [n][4] / ctl [n][2] followed by the next coupling; img / pred [2B, rows, C], source branches first,
// z / x0 bf16 and acc fp32 dense [B, rows, C].  The step launcher does not see the row: a caller that passes acc == NULL vouches that every
// row it runs has first and apply set
int fluxmi_k_flowedit_couple(void* img, const void* z, const void* x0, float t, float one_minus_t, const unsigned* ids, unsigned eval, int B,
                             long long img_rows, long long pred_rows, int c_in, int c_out, hipStream_t s);
int fluxmi_k_flowedit_step(void* img, const void* pred, void* z, float* acc, const void* x0, const float* coef, const int* ctl, const int* step,
                           const unsigned* ids, const int* eval_offset, int B, long long img_rows, long long pred_rows, int c_in, int c_out,
                           hipStream_t s);
// Tiled generation (window_step.hip; include/fluxmi.h, fluxmi_window_gather / _step): the canvas bf16 [N, Hc, Wc, C] beside a stream of
// N * ny * nx windows of h x w tokens (2x when guided: scale != NULL / guided != 0), row0 / col0 / Ny / Nx DEVICE tables.  The launchers do not
// see the tables (the kernel never leaves the stream whatever they hold): fluxmi_window_check_tables applies the placement rules to HOST copies
int fluxmi_k_window_gather(const void* canvas, void* img, const int* row0, const int* col0, int N, int Hc, int Wc, int h, int w, int ny, int nx,
                           int C, int guided, hipStream_t s);
int fluxmi_k_window_step(void* canvas, void* img, const void* pred, const float* dts, const int* step, const float* scale, const int* row0,
                         const int* col0, const float* Ny, const float* Nx, int N, int Hc, int Wc, int h, int w, int ny, int nx, int C,
                         hipStream_t s);
int fluxmi_window_check_tables(const char* who, const int* row0, const int* col0, int Hc, int Wc, int h, int w, int ny, int nx);
// first-block step cache (elementwise.hip): streaming passes over B samples of n bf16 elements, x side strided, cache side dense
int fluxmi_k_fb_snapshot(const void* x, long long x_bstride, void* dst, int B, long long n, hipStream_t s);
int fluxmi_k_fb_commit(const void* x, long long x_bstride, const void* r, void* r_ref, void* h1, int B, long long n, hipStream_t s);
int fluxmi_k_fb_metric(const void* x, long long x_bstride, const void* h0, void* r, const void* r_ref, float* part, float* ratio,
                       float* numden, int B, long long n, hipStream_t s);
int fluxmi_k_fb_store(const void* x, long long x_bstride, const void* h1, void* R, int B, long long n, hipStream_t s);
int fluxmi_k_fb_apply(void* x, long long x_bstride, const void* h1, long long h1_bstride, const void* R, int B, long long n, hipStream_t s);
// guidance shaping of true CFG (guidance.hip; include/fluxmi.h, fluxmi_guidance_moments / _combine): nine per-image sums over (c, u, r) as
// per-workgroup partials, then p = alpha c + beta u + gamma r with fp64-derived per-image coefficients written to both halves of pred
int fluxmi_k_guidance_moments(const void* pred, const float* r, float* part, int B, long long N, hipStream_t s);
int fluxmi_k_guidance_combine(void* pred, float* r, const float* part, const float* params, const int* step, const int* step_offset,
                              float* coef_out, int B, long long N, hipStream_t s);
// latent preview (preview.hip; include/fluxmi.h, fluxmi_latent_preview): x0 = x - t v of one evaluation projected 16 -> 3 into a ring slot chosen
// on the device from *step and ctl = {every, eval_offset}
int fluxmi_k_latent_preview(const void* x, const void* pred, const float* ts, const int* step, const float* scale, const float* proj,
                            const int* ctl, void* out, int B, long long img_rows, long long pred_rows, int c_in, int c_out, int h, int w,
                            hipStream_t s);
// ControlNet residual hand-over: x[b, j] = bf16(x[b, j] + bf16(r[b, j] * *s_dev)), B samples of n elements, batch strides in elements
int fluxmi_k_add_scaled(void* x, long long x_bstride, const void* r, long long r_bstride, const float* s_dev, int B, long long n, hipStream_t s);
// IP-Adapter term of a double block (ip_attention.hip; include/fluxmi.h, fluxmi_ip_attention): scale == NULL writes o, else x += bf16(o * scale[b])
int fluxmi_k_ip_attention(const void* qkv, long long ld_qkv, long long qkv_bstride, const void* qn_scale, const void* k_ip, const void* v_ip,
                          long long kv_bstride, void* out, long long ld_o, long long o_bstride, const float* scale, long long scale_bstride,
                          int B, int rows, int heads, int Nk, hipStream_t s);
int fluxmi_k_set_timestep(void* t_vec, const float* ts, const int* step, int B, hipStream_t s);
int fluxmi_k_advance_step(int* step, hipStream_t s);
int fluxmi_k_clock_sample(unsigned long long* out2, hipStream_t s);
int fluxmi_k_im2col3x3(const void* x, void* col, int B, int H, int W, int C, int up, hipStream_t s);
int fluxmi_k_im2col3x3_s2(const void* x, void* col, int B, int Hi, int Wi, int C, hipStream_t s);
int fluxmi_k_groupnorm(const void* x, const void* gamma, const void* beta, void* y, float* work, int B, int P, int C, int swish, float eps,
                       hipStream_t s);
int fluxmi_k_softmax_rows(const void* S, void* P, int rows, int cols, long long ld, float scale, hipStream_t s);
int fluxmi_k_row_norm(const void* x, const void* w, const void* b, void* y, int rows, int D, long long ldx, long long ldy, float eps, int mode,
                      hipStream_t s);
int fluxmi_k_act_mul(const void* in, void* out, int rows, int F, long long ld_in, long long ld_out, int mode, hipStream_t s);
int fluxmi_k_text_attention(const void* q, const void* k, long long ld_qk, const void* vt, long long ld_vt, void* out, long long ld_out,
                            const float* rel_bias, int bias_ld, const void* v_bias, float scale, int causal, int L, int Lp, int H, hipStream_t s);
int fluxmi_k_vae_attention(const void* q, const void* k, long long ld_qk, long long bs_qk, const void* vt, long long ld_vt, long long bs_vt,
                           void* out, long long ld_out, long long bs_out, const void* v_bias, int D, int P, int Pp, int B, hipStream_t s);
int fluxmi_k_conv3x3_dense(const void* x, long long ldx, int Cin, const void* w2, const void* bias, void* out, long long ldo, int Cout,
                           const void* r1, long long ldr1, float a1, const void* r2, long long ldr2, float a2, float slope, int act,
                           int upsample, int B, int H, int W, hipStream_t s);
// control-map preprocessors (preprocess.hip; include/fluxmi.h, fluxmi_canny* / fluxmi_rgb_to_gray / fluxmi_gaussian_blur): uint8 NHWC images with
// row and image strides in bytes
int fluxmi_k_canny_classify(const void* rgb, long long ld, long long bs, void* state, long long sld, long long sbs, int B, int H, int W,
                            int low, int high, int l2, hipStream_t s);
int fluxmi_k_canny_hysteresis_round(void* state, long long sld, long long sbs, int B, int H, int W, int* changed_flag, hipStream_t s);
int fluxmi_k_canny_hysteresis(void* state, long long sld, long long sbs, void* edges, long long eld, long long ebs, int* flags, int B, int H,
                              int W, int* rounds_out, hipStream_t s);
int fluxmi_k_canny(const void* rgb, long long ld, long long bs, void* edges, long long eld, long long ebs, void* work, long long work_bytes,
                   int B, int H, int W, int low, int high, int l2, int* rounds_out, hipStream_t s);
int fluxmi_k_rgb_to_gray(const void* rgb, long long ld, long long bs, void* gray, long long gld, long long gbs, int B, int H, int W,
                         hipStream_t s);
int fluxmi_k_gaussian_blur(const void* src, long long ld, long long bs, void* dst, long long dld, long long dbs, void* work, long long work_bytes,
                           int B, int H, int W, int C, float sigma, hipStream_t s);
// the baseline JPEG encoder (include/fluxmi.h, fluxmi_jpeg_*): the host's plan of one encode (jpeg_host.cpp: geometry, the layout of `work`,
// the scaled quantisation tables, the header bytes) and the launches that run it (jpeg.hip)
struct FluxmiJpegPlan {
  int H, Hs, W, ss, bpm;       // image rows, stacked rows B * H, columns, FLUXMI_JPEG_420 / _444, blocks per MCU (6 / 3)
  int mw, mh, nbw, nbh;        // MCUs across / down, 8 x 8 blocks that hold image pixels across / down
  int R;                       // MCUs per interval as run: `restart`, or every MCU when restart = 0
  long long n_mcu, n_int;      // MCUs, intervals = ceil(n_mcu / R)
  long long stride;            // bytes of one interval's slot
  long long off_sizes, off_offs, off_slots, work_bytes, out_cap;
  int hdr_bytes;
  unsigned char hdr[640];      // SOI .. SOS
  unsigned char q[2][64];      // the scaled tables, ZIGZAG order: [0] luminance, [1] chrominance
};
int fluxmi_jpeg_plan(const char* who, int B, int H, int W, int quality, int subsampling, int restart, FluxmiJpegPlan* p);
int fluxmi_k_jpeg_encode(const FluxmiJpegPlan& p, const void* rgb, long long ld, long long bs, void* work, void* out, long long out_cap,
                         void* n_bytes_dev, hipStream_t s);
int fluxmi_k_vision_attention(const void* q, const void* k, long long ld_qk, long long bs_qk, const void* vt, long long ld_vt, long long bs_vt,
                              void* out, long long ld_out, long long bs_out, const void* v_bias, float scale, int head_dim, int L, int Lp, int H,
                              int B, hipStream_t s);
int fluxmi_k_patchify(const void* pix, void* out, int B, int C, int H, int W, int P, int G, int Kp, hipStream_t s);
int fluxmi_k_patchify_rect(const void* pix, void* out, int B, int C, int H, int W, int P, int Gh, int Gw, int Kp, hipStream_t s);
// the Depth Anything estimator's own kernels (depth.hip; include/fluxmi.h has the arithmetic): NHWC bf16 maps behind one pixel stride
int fluxmi_k_unary(const void* x, void* y, long long rows, int cols, long long ld_in, long long ld_out, int kind, hipStream_t s);
int fluxmi_k_resize_bilinear(const void* x, long long ldx, void* out, long long ldo, const void* add, long long lda, int B, int Hi, int Wi,
                             int Ho, int Wo, int C, hipStream_t s);
int fluxmi_k_depth_head(const void* x, long long ldx, int C, const void* w, const void* bias, float* out, long long n, hipStream_t s);
int fluxmi_k_depth_to_map(const float* depth, long long ld, long long bs, void* out, long long out_ld, long long out_bs, float* work,
                          long long work_bytes, int B, int h, int w, int H, int W, int normalize, hipStream_t s);
int fluxmi_k_qkv_rope(const void* qkv, long long ld, const void* pe, const void* q_scale0, const void* k_scale0,
                      const void* q_scale1, const void* k_scale1, void* Q, void* K, void* VT, int B, int L, int Lp, int H,
                      int split, int k_f16, hipStream_t s);
int fluxmi_k_attention(const void* Q, const void* K, const void* VT, void* out, long long ld_out, int col_off, int out_fp8,
                       const float* q_scale0, const float* q_scale1, int split, int B, int L, int Lp, int H, int fmt, hipStream_t s,
                       const void* qraw = nullptr, long long ldq = 0, const void* pe = nullptr, const void* qn0 = nullptr,
                       const void* qn1 = nullptr, int k_f16 = 0, int out_pairs = 0, const void* groups = nullptr);
