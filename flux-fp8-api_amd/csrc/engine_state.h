// fluxmi -- the engine's state: what engine.hip (create, prepare, the forward and its blocks, ControlNet / IP-Adapter plumbing, diagnostics)
// and engine_denoise.hip (request state, side allocations, the stepper, graph capture, the denoise entry points) share.  Internal to csrc.
#pragma once
#include <string.h>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "common.h"
#include "fluxmi_internal.h"

constexpr int MAX_STEPS = 1024;
// samples per engine pass: bounds the workspace (1.1 GB per 1024x1024 sample) and the step-ahead modulation table (2.1 MB per step and
// sample); the host wrapper runs larger batches as equal consecutive passes
constexpr int FLUXMI_ENGINE_MAX_BATCH = 32;
constexpr int MODS_STEPS = 64;  // steps per window of the step-ahead modulation table; a longer request rebuilds the table every MODS_STEPS steps
struct Buf { void* p; size_t n; };
typedef fluxmi_engine E;

// What a captured piece bakes in beside the kernel choices (StepGraphs::gen): launches and launch arguments.  Everything else a request
// brings is device data.  Two requests share pieces exactly when their keys are equal; step_key (engine_denoise.hip) builds a key in zeroed
// memory, padding included, with every field a request does not use at zero, so that keys compare as bytes.
struct StepKey {
  bool cfg;        // the update kind (`warmed` and the pieces): guided or plain -- the two never share a graph
  bool masked;     // the attention kind: token-group masked or dense launches are baked into the pieces like the update kernel
  bool blend;      // the update kind, continued: the masked-latent blend kernel instead of the (guided) Euler kernel ...
  bool diff;       // ... and its differential form (the threshold table is a launch argument)
  bool solver;     // ... and the table-driven solver update (fluxmi_engine_set_solver): WHICH solver is device data, not a kind
  bool noise;      // ... and its form with the noise term (fluxmi_engine_set_solver_noise): seeds and the offset are device data
  bool edit;       // ... and FlowEdit's update (fluxmi_engine_denoise_edit): tables, ids, offset and the guidance pair are device data ...
  const void* fe_acc;  // ... its fp32 accumulator is a launch argument: null until a program that averages has made the buffer, and unless the call is an edit call
  bool win;        // ... and the windowed update (fluxmi_engine_denoise_windows): tables and scale are device data; the canvas geometry, which
  int win_geo[7];  // ... is a launch argument, and the canvas's address are part of the key (zero / null unless the call is windowed)
  const void* win_x;
  bool shaped;     // guidance shaping (fluxmi_engine_set_guidance) on a guided call: two launches in front of the guided update; mode and values are device data
  bool previewed;  // the preview launch in front of the update (fluxmi_engine_set_preview, every > 0): cadence, offset and factors are device data ...
  int pv_h, pv_w;  // ... the token grid is a launch argument (zero unless previewed)
  const void* cn;  // the attached ControlNet whose launches (and workspace pointers) are baked into the pieces, or none ...
  unsigned long long cn_gen;  // ... and the generation of its workspace / weight binding: process-wide unique, so a net created at a freed net's address never matches
  const void* ip;  // the IP-Adapter's K / V buffer baked into the pieces (null: no adapter launches), its Nk ...
  int ip_nk;
  unsigned long long ip_gen;  // ... and the buffer's generation (an allocation at a freed buffer's address never matches)
};
inline bool operator!=(const StepKey& a, const StepKey& b) { return memcmp(&a, &b, sizeof(StepKey)) != 0; }

// The captured pieces of one kind of frozen step (plain: the whole step; cached: head, body, skip) and what they were captured for.  Kernel
// choices and the update kernel are baked into a captured piece, so the set is keyed on the tuning generation and the request's StepKey.
struct StepGraphs {
  hipGraphExec_t exec[3] = {nullptr, nullptr, nullptr};
  bool ok = false;      // exec[] is instantiated and replayable
  bool warmed = false;  // one frozen step of this kind, shape and key has run eagerly (lazy one-time inits done): the next call may capture at once
  unsigned gen = 0;     // fluxmi_tuning_generation() the pieces were captured under
  StepKey key = {};     // ... and the request they were captured (or warmed) for
  void drop() {
    for (hipGraphExec_t& g : exec)
      if (g) { hipGraphExecDestroy(g); g = nullptr; }
    ok = warmed = false;
  }
};

// One side allocation of a prepared shape: device memory that a feature makes when its first request arrives -- a request without the feature
// allocates none of it -- and that is dropped with the workspace.  Its items are 256-byte aligned and registered in fluxmi_engine::bufs under
// their names (a null name: not registered).  fluxmi_engine_workspace_bytes counts every one of them.
struct SideItem { const char* name; size_t bytes; };
struct SideBuf {
  char* p = nullptr;
  size_t bytes = 0;
  // hipMalloc of exactly `total` bytes, zeroed on `s` if `zero`; a failure is "<who>: hipMalloc(<total> bytes) failed<what>"
  int alloc(size_t total, bool zero, hipStream_t s, const char* who, const char* what);
  // the allocation for `items`, made if there is none, and the items' names registered
  int ensure(E* e, std::initializer_list<SideItem> items, bool zero, hipStream_t s, const char* who, const char* what);
  void drop(E* e);  // frees the memory and erases its names
};
// (the comments beside the engine's feature state say what each one holds)
enum { SB_FB = 0, SB_INP, SB_SOL, SB_SOL_IDS, SB_GD, SB_PV, SB_FE, SB_FE_Z, SB_FE_ACC, SB_WIN, SB_IP, SB_COUNT };

// FlowEdit's device tables, the workspace buffer "fe_tab": the program's rows, then the noise ids of the B / 2 images with the evaluation
// offset behind them (one copy).  Staged through SchedStaging::fe, which is the same layout.
struct FeTab {
  float coef[MAX_STEPS * 4];
  int ctl[MAX_STEPS * 2];
  struct Draw { unsigned ids[FLUXMI_ENGINE_MAX_BATCH * 4]; int offset; } draw;
};
constexpr size_t FE_TAB_BYTES = (size_t)MAX_STEPS * 6 * 4 + (size_t)FLUXMI_ENGINE_MAX_BATCH * 16 + 4;
static_assert(sizeof(FeTab) == FE_TAB_BYTES, "FeTab must keep the layout of the fe_tab buffer");

// The pinned host staging of one denoise call's tables (fluxmi_engine::h_sched): every table goes to the device from here, so that the call
// never waits on the stream.  Every member is 4 bytes wide: no padding.
struct SchedStaging {
  float ts[MAX_STEPS + 1], dts[MAX_STEPS + 1];                           // the schedule
  float tnext[MAX_STEPS + 1], omt[MAX_STEPS + 1], thr[MAX_STEPS + 1];    // inpainting: the next time of every step, its complement, the thresholds
  float sol_coef[MAX_STEPS * 8];                                         // the solver program
  int sol_ctl[MAX_STEPS * 4];
  unsigned sol_ids[FLUXMI_ENGINE_MAX_BATCH * 4 + 1];                     // the noise ids [B][4] of the prepared batch B, the evaluation offset right behind them
  struct { float params[8]; int offset; } gd;                            // guidance shaping: "gd_params" and the step offset behind it
  struct { float proj[51]; int ctl[2]; } pv;                             // previews: "pv_proj", "pv_ctl" {every, eval_offset}
  FeTab fe;                                                              // FlowEdit: "fe_tab"
};
static_assert(sizeof(SchedStaging) == (5 * (MAX_STEPS + 1) + 12 * MAX_STEPS + 4 * FLUXMI_ENGINE_MAX_BATCH + 1 + 9 + 53 + 6 * MAX_STEPS +
                                       4 * FLUXMI_ENGINE_MAX_BATCH + 1) * sizeof(float),
              "SchedStaging must keep the size of the staging buffer it replaced");

struct fluxmi_engine {
  fluxmi_model_desc_t d;
  std::vector<fluxmi_linear_t> lin;
  std::vector<const void*> norm;
  int i_img_in, i_time_in, i_vec_in, i_guid_in, i_txt_in, i_double0, i_single0, i_final_mod, i_final_lin;
  int B = 0, Li = 0, Lt = 0, L = 0, Lp = 0;
  int Lpred = 0;  // predicted (and stepped) rows per sample: the leading rows of the image stream; Li - Lpred = Lc reference rows (Kontext)
  long long mod_cols = 0;
  char* ws = nullptr;
  size_t ws_bytes = 0;
  std::map<std::string, Buf> bufs;
  SideBuf side[SB_COUNT];          // the features' own allocations (SB_*), made by their first request and dropped with the workspace
  // persistent small device state
  char* consts = nullptr;
  float *d_freqs, *d_omega, *d_ts, *d_dts, *d_amax, *d_amax_own;
  int *d_axis, *d_step;
  FluxmiCalibLayer* d_calib;
  FluxmiGemvLayer* d_gemv = nullptr;
  std::vector<FluxmiGemvLayer> h_gemv;
  std::vector<FluxmiCalibLayer> h_calib_mod;  // modulation layers that share silu(vec)
  FluxmiCalibLayer* d_calib_mod = nullptr;
  int gemv_blocks = 0, gemv_maxK = 0;
  // step-ahead modulation table (frozen scales): every modulation vector of every remaining step of a request, computed
  // before the loop in batches of 8 steps so that the 3.2 GB of modulation weights are streamed once per 8 steps, not per step
  char* mods_all = nullptr;
  size_t mods_all_bytes = 0;
  int mods_step0 = 0;
  bool mods_table = false;  // the step being sequenced takes its modulations from the table
  bool qlut_valid = false;  // the quantising-epilogue tables reflect the current input scales
  // the frozen step's graphs: the plain step (one piece) and the step-cache step (head, body, skip).  Separate sets, so that plain and cached
  // requests alternating on one shape never re-capture; both go stale by ONE rule (graphs_stale) and run through ONE loop (frozen_steps)
  StepGraphs step_graphs, fb_graphs;
  bool txt_emb_valid = false;
  // row-pair copies of the F8Linear weights the persistent GEMM launches read (fluxmi_gemm_group_t.W_pairs): one allocation, offsets per linear
  // (-1 = none); rebuilt on the first launch after create / rebind (the weights may have been rewritten: LoRA fuse)
  char* pairs = nullptr;
  size_t pairs_bytes = 0;
  std::vector<long long> pairs_off;
  bool pairs_dirty = true;
  bool pairs_skipped = false;      // the copies were wanted and did not fit (ensure_pairs): retried at the next prepare
  unsigned pairs_gen = 0;          // fluxmi_tuning_generation() the copies were built under (fluxmi_tuning_t.w_pairs may have changed)
  float* d_cfg = nullptr;          // true-CFG scale (device scalar, like d_dts: one guided graph serves every scale)
  // token-group attention mask (fluxmi_engine_set_attn_groups): every attention launch of a forward reads the [B, L] descriptors in the
  // workspace buffer "attn_groups".  The CONTENTS are device data -- one set of graphs serves every table of a prepared shape -- masked
  // versus dense is a graph kind (graphs_stale).  Cleared when the workspace is re-allocated: a table belongs to a shape
  bool masked = false;
  int* d_step0 = nullptr;          // first step of the modulation table (device scalar: the captured graph reads it)
  // the layout each fp8 activation buffer (ACT_A8 .. ACT_CAT8) was last written in: true = row pairs (fused mode, act_pairs), false = plain
  // rows.  Set by the stages that write them (and by a replayed step graph); fluxmi_engine_copy_buffer converts by it
  bool act_in_pairs[4] = {false, false, false, false};
  int mods_rows_cap = 0;           // rows (steps x B) the table holds; sized in engine_prepare, never inside denoise
  // pinned host staging for the tables of a denoise call (SchedStaging: schedule, inpainting, solver, noise ids, shaping, preview, FlowEdit),
  // guarded by an event so that engine_denoise never waits on the stream
  SchedStaging* h_sched = nullptr;
  hipEvent_t ev_sched = nullptr;
  bool sched_pending = false;
  // hipEvent timing of the frozen (graph-replayed) part of the last denoise call, read back by fluxmi_engine_last_timing
  hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;
  int timed_steps = 0;
  // multi-GPU calibration: caller-owned amax array + host hook called between the amax reduction of a layer and its scale update
  float* amax_ext = nullptr;
  fluxmi_amax_hook_t amax_hook = nullptr;
  void* amax_user = nullptr;
  // first-block step cache (fluxmi_engine_set_step_cache).  Threshold, hit counter and log are HOST state: one set of
  // graphs (fb_graphs) serves every threshold.  The buffers (h0 | r, h1, r_ref, R, partial sums, ratios) are one allocation (SB_FB) made at the first cached
  // call of a prepared shape and dropped with the workspace; a plain request never allocates, captures or launches any of this.
  float fb_threshold = 0.f;
  int fb_max_hits = 0;
  float* h_ratio = nullptr;        // pinned: the B ratios of the step, copied out behind the head piece
  hipEvent_t ev_fb = nullptr;      // ... and the event the host waits on before it decides
  int fb_log_B = 0;
  std::vector<float> fb_log_ratio;          // [frozen steps of the last call][B]
  std::vector<unsigned char> fb_log_hit;    // [frozen steps of the last call]
  // masked-latent inpainting (fluxmi_engine_set_inpaint).  The buffers (x0 | noise | mask, each bf16 [B, Lpred, C_out]: room
  // for a plain call's B images) are one allocation (SB_INP) made at the first masked call of a prepared shape and dropped with the workspace; the
  // per-step tables ride in the constants block and the pinned schedule staging.  A request without a mask allocates and launches none of it.
  bool inp_on = false, inp_diff = false;
  int inp_B = 0;                   // the caller's images the buffers hold
  std::vector<double> inp_thr;     // differential thresholds, one per step of the following denoise call
  float *d_tnext = nullptr, *d_omt = nullptr, *d_thr = nullptr;
  // solver program (fluxmi_engine_set_solver): the host tables of the following denoise calls, their device copies
  // (an allocation of their own, staged through h_sched like dts), and the saved iterate / two fp32 history slots (SB_SOL: xs bf16 | hist fp32 [2], each
  // [B, Lpred, C_out]) made at the first solver call of a prepared shape and dropped with the workspace.  Nothing of it without a solver.
  bool sol_on = false;
  int sol_n = 0;
  std::vector<float> sol_coef;     // [sol_n][8]
  std::vector<int> sol_ctl;        // [sol_n][4]
  float* d_sol_coef = nullptr;
  int* d_sol_ctl = nullptr;
  SideBuf sol_tab;                 // ... their allocation (like the constants block, not counted as workspace)
  // the noise of a stochastic program (fluxmi_engine_set_solver_noise): the host ids [sol_noise_B][4] and the evaluation offset of the
  // following denoise calls; their device copy "sol_ids" (SB_SOL_IDS: uint32 [B][4] | the offset, staged through h_sched like the tables) is made at
  // the first noise call of a prepared shape and dropped with the workspace.  Nothing of it without noise.
  bool sol_noise = false;
  int sol_noise_B = 0, sol_eval_offset = 0;
  std::vector<unsigned> sol_ids;
  // guidance shaping (fluxmi_engine_set_guidance): the host parameters and step offset of the following guided denoise
  // calls; their device copy "gd_params" (float [8] | the offset, staged through h_sched like the schedule), the moments' partials "gd_part",
  // the last step's coefficients "gd_coef" and APG's running difference "gd_r" (fp32 [B / 2][Lpred * C_out]) are one allocation (SB_GD) made at the
  // first shaped call of a prepared shape and dropped with the workspace.  Nothing of it without shaping.
  bool gd_on = false;
  bool gd_zero_r = false;          // a set call came in: the next guided denoise call zeroes "gd_r" on its stream
  float gd_params[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int gd_offset = 0;
  // FlowEdit (fluxmi_engine_set_flow_edit / _denoise_edit): the host tables, ids, offset and guidance pair of the following
  // edit calls.  Device side, three allocations dropped with the workspace: SB_FE = "fe_x0" (bf16 [B / 2, Lpred, C_out], filled by the set
  // call) | "fe_tab" (FeTab, staged through h_sched like the solver's), SB_FE_Z = "fe_z" made by the first edit call of a prepared shape,
  // SB_FE_ACC = "fe_acc" (fp32) made by the first edit call whose
  // program has a row without first or apply.  Nothing of it without an edit request.  fe_call: the running denoise call is an edit call.
  bool fe_on = false, fe_call = false, fe_need_acc = false;
  int fe_B = 0, fe_n = 0, fe_eval_offset = 0;
  float fe_gs = 0.f, fe_gt = 0.f;
  std::vector<float> fe_coef;      // [fe_n][4]
  std::vector<int> fe_ctl;         // [fe_n][2]
  std::vector<unsigned> fe_ids;    // [fe_B][4]
  // Tiled generation (fluxmi_engine_set_windows / _denoise_windows): the geometry {N, Hc, Wc, h, w, ny, nx} of the
  // following windowed calls.  Device side, one allocation dropped with the workspace: SB_WIN = "win_x" (the canvas, bf16 [N, Hc, Wc, C]) |
  // "win_tab" (row0 int [ny] | col0 int [nx] | Ny fp32 [ny][Hc] | Nx fp32 [nx][Wc], each 256-byte aligned, filled by the set call).  Nothing
  // of it without a windowed request.  win_call: the running denoise call is a windowed call.
  bool win_on = false, win_call = false;
  int win_geo[7] = {0, 0, 0, 0, 0, 0, 0};
  size_t win_off[4] = {0, 0, 0, 0};  // the four tables' offsets in "win_tab"
  // ControlNet (fluxmi_controlnet_create / fluxmi_engine_attach_controlnet).  A net is an engine of its own kind
  // (is_cn): no final layer, the controlnet_* projections behind the trunk's linears, the residuals of a forward in its workspace buffer
  // "cn_res" [Nd + Ns][B, Li, H].  The main engine holds the attached net (cn) and the conditioning scale (d_cn_scale, device data).
  bool is_cn = false;
  int i_cn_x = -1, i_cn_d0 = -1, i_cn_s0 = -1;   // controlnet_x_embedder, controlnet_blocks[0], controlnet_single_blocks[0]
  const void* cn_mode_table = nullptr;           // controlnet_mode_embedder.weight bf16 [cn_num_mode, H] (Union), or none
  int cn_num_mode = 0;
  int txt_extra = 0;               // 1: row 0 of the text stream is the mode embedding (Lt = the request's text rows + 1)
  int cn_trial = 0;                // the net's own calibration counter
  // a number no other engine state of this process ever had (next_generation): renewed at create, when the workspace is dropped and when the
  // weights are re-bound.  Step graphs that baked a net in are keyed on it, never on the net's address alone (the allocator reuses addresses)
  unsigned long long ws_gen = 0;
  fluxmi_engine* cn = nullptr;        // main: the attached net
  fluxmi_engine* cn_owner = nullptr;  // net: the main engine it is attached to
  int cn_batch = 0;                // main: the caller's images the attached cond holds
  float* d_cn_scale = nullptr;
  // IP-Adapter (fluxmi_engine_set_ip_adapter): the step-invariant keys / values of every double block and the
  // per-sample, per-block scales in ONE engine-owned allocation (SB_IP: k | v, each bf16 [depth][B][Nk][H], then scales fp32 [B][depth]) made by the
  // set call -- never inside a capture -- kept while it is large enough and dropped with the workspace.  Contents are device data; on / off,
  // the buffer and Nk are a kind of step graph.  Nothing of it without an adapter.
  bool ip_on = false;
  int ip_nk = 0, ip_B = 0;
  unsigned long long ip_gen = 0;
  std::vector<float> ip_scales_h;  // the staged scales' host copy (alive until the next set call: the source of an asynchronous copy)
  // progress, previews and cancellation (fluxmi_engine_set_preview): the host state of the following denoise calls.  The
  // device buffers ("pv_proj" float [51] | "pv_ctl" int {every, eval_offset} | "pv_out" uint8 [SLOTS][B][2 h][2 w][3]) are one allocation (SB_PV) made at
  // the first previewed call of a prepared shape and dropped with the workspace; proj and ctl are staged through h_sched like the schedule.
  // The pinned delivery buffer, the private copy stream and the event ring are made by the first set call with a hook and live as long as
  // the engine.  Nothing of it without a hook; with every = 0 only the events.
  fluxmi_step_hook_t pv_hook = nullptr;
  void* pv_user = nullptr;
  int pv_every = 0, pv_offset = 0, pv_n = 0, pv_h = 0, pv_w = 0;
  float pv_proj[51];
  unsigned char* pv_host = nullptr;
  size_t pv_host_bytes = 0;
  hipStream_t pv_stream = nullptr;
  hipEvent_t pv_ev[FLUXMI_PREVIEW_DEPTH + 1] = {};
  // ... and the state of the running call: evaluations launched / delivered to the hook, the caller's images, whether the hook said stop
  int pv_launched = 0, pv_delivered = 0, pv_images = 0;
  bool pv_cancelled = false;
  long long captures = 0;          // graph captures since create (fluxmi_engine_preview_stats: read-only, for tests)
};

template <class T> T* buf(E* e, const char* name) {
  auto it = e->bufs.find(name);
  return it == e->bufs.end() ? nullptr : (T*)it->second.p;
}

// ---- engine.hip: what the denoise loop runs -------------------------------------------------------------------------------------------------
// Phases [p0, p1] of the forward: 0 = embedders + modulation vectors, 1 = double block 0, 2 = every later block, 3 = final layer.  The step
// cache cuts the frozen step between them (head = 0..1, body = 2..3, skip = 3); every other caller runs 0..3, the launches it always ran.
enum { PH_EMBED = 0, PH_BLOCK0 = 1, PH_BLOCKS = 2, PH_FINAL = 3 };
unsigned long long next_generation();
bool act_pairs(const E* e, bool fused);
int ensure_pairs(E* e, hipStream_t s);
int embed_txt(E* e, const u16* txt, bool calib, int trial, u16* dst, long long dst_bstride, hipStream_t s);
int put_mode_row(E* e, u16* dst, long long dst_bstride, hipStream_t s);
int precompute_mods(E* e, int step0, int step_end, const u16* g_vec, const u16* y, hipStream_t s);
int build_qluts(E* e, hipStream_t s);
int c_out(const E* e);
bool all_block_linears_f8(E* e, int* blk = nullptr);
bool any_f8(const E* e);
int forward_impl(E* e, const u16* img, const u16* txt, const u16* y, const u16* t_vec, const u16* g_vec, u16* pred, int mode, int trial,
                 bool txt_cached, hipStream_t s, int p0 = PH_EMBED, int p1 = PH_FINAL);
int cn_forward(E* e, const u16* img, const u16* txt, const u16* y, const u16* t_vec, const u16* g_vec, int mode, int trial, bool table, hipStream_t s);
int frozen_forward(E* e, int mode, const u16* g_arg, int p0, int p1, hipStream_t s);
int cn_usable(E* e);
int ip_usable(E* e);
void scope_set(E* e);
// the engine's split-K scratch and its scratch for attention's balanced grid, for every launch of this thread while an engine entry point runs; a
// prefetch left pending by an error return between set_pf and its launch is dropped on entry and on exit (it points into weights the caller may free)
struct SplitkScope {
  explicit SplitkScope(E* e) { scope_set(e); }
  ~SplitkScope() {
    fluxmi_gemm_set_batch(1);
    fluxmi_set_splitk_scratch(nullptr);
    fluxmi_set_attn_scratch(nullptr);
    fluxmi_set_prefetch(nullptr);
  }
};
