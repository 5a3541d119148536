// fluxmi -- the denoise loop of the engine (engine.hip has the forward it steps): the request state set by the fluxmi_engine_set_* calls, the
// side allocations a feature's first request makes, the frozen-step loop with its graph capture, the preview look-ahead, and the four
// denoise entry points.  Host code only: every kernel it launches lives in another file.
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <dlfcn.h>
#include <functional>

#include "engine_state.h"

// ---- side allocations ---------------------------------------------------------------------------------------------------------------------------
static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

int SideBuf::alloc(size_t total, bool zero, hipStream_t s, const char* who, const char* what) {
  if (hipMalloc((void**)&p, total) != hipSuccess) {
    (void)hipGetLastError();
    p = nullptr;
    fluxmi_set_error("%s: hipMalloc(%zu bytes) failed%s", who, total, what);
    return 2;
  }
  bytes = total;
  if (zero) FLUXMI_CHECK_HIP(hipMemsetAsync(p, 0, total, s));
  return 0;
}
int SideBuf::ensure(E* e, std::initializer_list<SideItem> items, bool zero, hipStream_t s, const char* who, const char* what) {
  size_t total = 0;
  for (const SideItem& it : items) total += up256(it.bytes);
  if (!p) FLUXMI_TRY(alloc(total, zero, s, who, what));
  size_t off = 0;
  for (const SideItem& it : items) {
    if (it.name) e->bufs[it.name] = Buf{p + off, it.bytes};
    off += up256(it.bytes);
  }
  return 0;
}
void SideBuf::drop(E* e) {
  if (!p) return;
  for (auto it = e->bufs.begin(); it != e->bufs.end();)
    it = (char*)it->second.p >= p && (char*)it->second.p < p + bytes ? e->bufs.erase(it) : std::next(it);
  hipFree(p);
  p = nullptr; bytes = 0;
}

// the step cache's buffers for the prepared shape, made once a cached request arrives (a plain request's workspace stays what it was)
constexpr long long FB_CHUNK_ELEMS = 16384;  // elements per workgroup of the metric pass (elementwise.hip, FB_CHUNK vectors)
static int ensure_fb(E* e, hipStream_t s) {
  if (!e->h_ratio) FLUXMI_CHECK_HIP(hipHostMalloc((void**)&e->h_ratio, FLUXMI_ENGINE_MAX_BATCH * sizeof(float), hipHostMallocDefault));
  if (!e->ev_fb) FLUXMI_CHECK_HIP(hipEventCreateWithFlags(&e->ev_fb, hipEventDisableTiming));
  const size_t n = (size_t)e->Lpred * e->d.hidden, rows = (size_t)e->B * n * 2;
  const size_t chunks = (n + FB_CHUNK_ELEMS - 1) / FB_CHUNK_ELEMS;
  return e->side[SB_FB].ensure(e, {{"fb_h0", rows}, {"fb_h1", rows}, {"fb_rref", rows}, {"fb_R", rows}, {"fb_part", (size_t)e->B * chunks * 8},
                                   {"fb_ratio", (size_t)e->B * 3 * 4}}, true, s, "engine_denoise", " (step cache)");
}

// the solver's saved iterate and history slots of the prepared shape, made once a solver request arrives (like ensure_fb)
static int ensure_sol(E* e, hipStream_t s) {
  if (e->side[SB_SOL].p) return 0;
  // the device tables (coef [MAX_STEPS][8] | ctl [MAX_STEPS][4]): constants like d_dts, but made here and not in the constants block, so
  // that an engine that never sees a solver allocates what it allocated before; like the constants block, not counted as workspace
  if (!e->sol_tab.p) {
    FLUXMI_TRY(e->sol_tab.alloc((size_t)MAX_STEPS * 12 * 4, false, s, "engine_denoise", " (solver tables)"));
    e->d_sol_coef = (float*)e->sol_tab.p;
    e->d_sol_ctl = (int*)(e->d_sol_coef + (size_t)MAX_STEPS * 8);
  }
  const size_t elems = (size_t)e->B * e->Lpred * c_out(e);
  return e->side[SB_SOL].ensure(e, {{"sol_xs", up256(elems * 2)}, {"sol_hist", up256(2 * elems * 4)}}, true, s, "engine_denoise", " (solver buffers)");
}

// elements of FlowEdit's buffers of the prepared shape, for the B / 2 images an edit call of this shape steps: the init latent (beside the
// device tables; made by the set call, which fills it), the edit state, and the fp32 accumulator of a program that averages
static size_t fe_elems(const E* e) { return (size_t)std::max(1, e->B / 2) * e->Lpred * c_out(e); }

constexpr long long GD_CHUNK_ELEMS = 16384;  // elements per workgroup of guidance shaping's moments pass (guidance.hip, GD_CHUNK vectors)

// roctx ranges (rocprofv3 --marker-trace) around the phases of a denoise call, resolved at run time so that the library has no
// hard dependency on the profiler: fluxmi_tuning_t.roctx (FLUXMI_ROCTX=1) turns them on.
namespace {
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    if (!fluxmi_tuning().roctx) return;
    void* h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return;
    push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
    pop = (int (*)())dlsym(h, "roctxRangePop");
    if (!push || !pop) push = nullptr, pop = nullptr;
  }
};
Roctx& roctx() { static Roctx r; return r; }
struct Range {
  Range(const char* name) { if (roctx().push) roctx().push(name); }
  ~Range() { if (roctx().pop) roctx().pop(); }
};

// ---- the request ------------------------------------------------------------------------------------------------------------------------------
// One denoise call, described once at its top: the four entry points differ in the kind alone.  Guided: the prepared batch B is 2 Bh, samples
// [0, Bh) the prompt branch and [Bh, B) the negative branch of the caller's Bh images; the caller's img [Bh, ...] is copied into both halves of
// the stream, every forward runs on the B samples, and the guided update keeps the halves bit-identical.  Edit: the batch is 2 Bh as well --
// source branches, then target branches -- but the halves hold different latents, `img` is the caller's edit state z [Bh, ...], and the update
// is fluxmi_k_flowedit_step on "fe_z" / "fe_x0": the stream only carries the two model inputs the kernel rebuilds.  Windowed: `img` is the
// caller's canvas, the stream holds its windows (guided: in both halves).
enum ReqKind { RQ_PLAIN, RQ_GUIDED, RQ_EDIT, RQ_WINDOWED, RQ_WINDOWED_GUIDED };
struct Request {
  ReqKind kind;
  float guidance, cfg_scale;
  int n_steps;
  hipStream_t s;
  int images;      // the caller's images: the prepared batch, half of it for a guided or an edit call
  bool shaped;     // guidance shaping runs: a guided call with a shaping state set (an unguided call does not consult the state)
  bool hooked;     // a step hook is set: progress and cancellation ...
  bool previewed;  // ... and, with every > 0, the preview launch
  bool sol_noise;  // the solver update takes its noise form
  bool cfg() const { return kind == RQ_GUIDED || kind == RQ_WINDOWED_GUIDED; }
  bool edit() const { return kind == RQ_EDIT; }
  bool win() const { return kind == RQ_WINDOWED || kind == RQ_WINDOWED_GUIDED; }
};
Request make_request(const E* e, ReqKind kind, float guidance, float cfg_scale, int n_steps, void* stream) {
  Request rq{kind, guidance, cfg_scale, n_steps, (hipStream_t)stream, 0, false, false, false, false};
  if (!e) return rq;  // (refused by the first check)
  rq.images = rq.cfg() || rq.edit() ? e->B / 2 : e->B;
  rq.shaped = rq.cfg() && e->gd_on;
  rq.hooked = e->pv_hook != nullptr;
  rq.previewed = rq.hooked && e->pv_every > 0;
  rq.sol_noise = e->sol_on && e->sol_noise;
  return rq;
}

// ---------------------------------------------------------------------------------------------------------
// The frozen steps [step, n_steps) of a request: ONE loop (frozen_steps) for the plain step and for the step with first-block caching.  The
// two differ only in their Stepper: the pieces a step is cut into -- each piece is one captured graph -- and how a step is sequenced from them.
// ---------------------------------------------------------------------------------------------------------
typedef std::function<int(hipStream_t)> StepFn;
struct StepPiece { const char* name; StepFn run; };
struct Stepper {
  StepGraphs* g;
  const char* range;                    // roctx range around the steps
  int n_pieces;
  StepPiece piece[3];
  std::function<int(bool graph)> step;  // one step on the caller's stream: the pieces replayed (graph) or run eagerly
  std::function<int()> pre_warm;        // what precedes the eager warm step (may be empty)
};

// The key of the pieces this request would capture (engine_state.h, StepKey), built in place: padding and every field the request does not use are zero.
void step_key(const E* e, const Request& rq, StepKey& k) {
  memset(&k, 0, sizeof k);
  k.cfg = rq.cfg();
  k.masked = e->masked;
  k.blend = e->inp_on;
  k.diff = e->inp_on && e->inp_diff;
  k.solver = e->sol_on;
  k.noise = e->sol_noise;
  k.edit = e->fe_call;
  if (e->fe_call) k.fe_acc = e->side[SB_FE_ACC].p;  // (once made, the buffer rides in every edit launch: a row with first and apply ignores it)
  k.win = e->win_call;
  if (e->win_call) {
    memcpy(k.win_geo, e->win_geo, sizeof k.win_geo);
    k.win_x = e->side[SB_WIN].p;
  }
  k.shaped = rq.shaped;
  k.previewed = rq.previewed;
  if (rq.previewed) { k.pv_h = e->pv_h; k.pv_w = e->pv_w; }
  k.cn = e->cn;
  if (e->cn) k.cn_gen = e->cn->ws_gen;
  if (e->ip_on && e->side[SB_IP].p) {
    k.ip = e->side[SB_IP].p;
    k.ip_nk = e->ip_nk;
    k.ip_gen = e->ip_gen;
  }
}

// The ONE staleness rule of both graph sets.  Kernel choices are baked into a captured piece: never replay one captured under other knobs
// (the quantising-epilogue tables follow the knobs too).  The update kernel and everything else in the key are baked in as well, and
// `warmed` speaks of one key: requests of two kinds on one shape never share a graph or a warm step, whether or not a graph exists yet.  The
// old pieces stay allocated until the re-capture replaces them (behind its stream synchronisation).
void graphs_stale(E* e, StepGraphs& g, const Request& rq) {
  if (g.ok && g.gen != fluxmi_tuning_generation()) g.ok = g.warmed = e->qlut_valid = false;
  StepKey key;
  step_key(e, rq, key);
  if (key != g.key) g.ok = g.warmed = false;
  memcpy(&g.key, &key, sizeof key);
}

// Captures pieces[0 .. n) into g.exec[0 .. n) on a private non-blocking stream (the caller has synchronised its own).  The only place that
// captures and instantiates; the stream sits behind a guard, so that no error path keeps it.
static int capture_pieces(StepGraphs& g, const StepPiece* pieces, int n) {
  struct CaptureStream {
    hipStream_t s = nullptr;
    ~CaptureStream() { if (s) hipStreamDestroy(s); }
  } cs;
  FLUXMI_CHECK_HIP(hipStreamCreateWithFlags(&cs.s, hipStreamNonBlocking));
  for (int p = 0; p < n; ++p) {
    hipGraph_t graph = nullptr;
    hipError_t ce = hipStreamBeginCapture(cs.s, hipStreamCaptureModeThreadLocal);
    const int rc = ce == hipSuccess ? pieces[p].run(cs.s) : 0;
    if (ce == hipSuccess) ce = hipStreamEndCapture(cs.s, &graph);  // ends the capture of a failed piece as well
    if (g.exec[p]) { hipGraphExecDestroy(g.exec[p]); g.exec[p] = nullptr; }
    if (!rc && ce == hipSuccess) ce = hipGraphInstantiate(&g.exec[p], graph, nullptr, nullptr, 0);
    if (graph) hipGraphDestroy(graph);
    if (!rc && ce != hipSuccess) fluxmi_set_error("engine_denoise: capturing %s failed: %s", pieces[p].name, hipGetErrorString(ce));
    if (rc || ce != hipSuccess) return rc ? rc : 2;
  }
  g.ok = true;
  g.gen = fluxmi_tuning_generation();
  return 0;
}

// ---- the throttled loop of a hooked call (fluxmi.h, fluxmi_engine_set_preview) ---------------------------------------------------------------
// Evaluation k of the call goes to the hook: waits on the event recorded behind it, copies its preview slot -- if it has one -- to the pinned
// buffer on the private stream, waits for that copy, calls the hook on the caller's thread.  A non-zero return sets pv_cancelled.
static int pv_deliver(fluxmi_engine_t* e, int k) {
  FLUXMI_CHECK_HIP(hipEventSynchronize(e->pv_ev[k % (FLUXMI_PREVIEW_DEPTH + 1)]));
  const long long g = (long long)e->pv_offset + k;
  const unsigned char* rgb = nullptr;
  if (e->pv_every > 0 && g % e->pv_every == 0) {
    const size_t bytes = (size_t)e->pv_images * e->pv_h * e->pv_w * 4 * 3;
    const size_t slot = (size_t)((g / e->pv_every) % FLUXMI_PREVIEW_SLOTS);
    FLUXMI_CHECK_HIP(hipMemcpyAsync(e->pv_host, buf<unsigned char>(e, "pv_out") + slot * bytes, bytes, hipMemcpyDeviceToHost, e->pv_stream));
    FLUXMI_CHECK_HIP(hipStreamSynchronize(e->pv_stream));
    rgb = e->pv_host;
  }
  e->pv_delivered = k + 1;
  if (e->pv_hook(e->pv_user, (int)g, e->pv_n, rgb, e->pv_images, 2 * e->pv_h, 2 * e->pv_w) != 0) e->pv_cancelled = true;
  return 0;
}
// One evaluation of a denoise call, `run`, under the look-ahead rule: the ONE helper of the calibrating loop and of frozen_steps.  Without a
// hook it is `run` alone.  With one: before launching evaluation i >= DEPTH, every evaluation up to i - DEPTH not yet delivered is delivered,
// in order; a cancel there returns FLUXMI_CANCELLED with nothing further launched.  Behind the launch the evaluation's event is recorded: slot
// i % (DEPTH + 1) of the ring, last used by evaluation i - DEPTH - 1, which has been delivered.
static int pv_eval(fluxmi_engine_t* e, hipStream_t s, const std::function<int()>& run) {
  if (!e->pv_hook) return run();
  const int i = e->pv_launched;
  while (e->pv_delivered <= i - FLUXMI_PREVIEW_DEPTH) {
    FLUXMI_TRY(pv_deliver(e, e->pv_delivered));
    if (e->pv_cancelled) return FLUXMI_CANCELLED;
  }
  FLUXMI_TRY(run());
  FLUXMI_CHECK_HIP(hipEventRecord(e->pv_ev[i % (FLUXMI_PREVIEW_DEPTH + 1)], s));
  e->pv_launched = i + 1;
  return 0;
}

// The modulation vectors of up to MODS_STEPS steps are produced ahead (one pass over the 3.2 GB of modulation weights per window); the table
// address and the device-side window origin never change, so ONE set of captured pieces serves every step of every request.  The first frozen
// step of a shape and key runs eagerly, so that every lazy one-time init (function attributes) happens outside capture; the steps
// behind it are replayed (use_graph) or run eagerly.  *first_timed = the first step behind ev_t0.
int frozen_steps(E* e, const Stepper& st, int mode, const Request& rq, int step, const u16* g_arg, int use_graph, int* first_timed) {
  hipStream_t s = rq.s;
  const int n_steps = rq.n_steps;
  StepGraphs& g = *st.g;
  bool t0 = false;
  while (step < n_steps) {
    const int win_end = std::min(n_steps, step + MODS_STEPS);
    {
      Range r("step-ahead modulation table");
      FLUXMI_TRY(precompute_mods(e, step, win_end, g_arg, buf<u16>(e, "y_s"), s));
      if (e->cn) {  // the attached ControlNet's own table, from the same schedule, guidance and y
        scope_set(e->cn);
        const int rc = precompute_mods(e->cn, step, win_end, e->cn->d.guidance_embed ? buf<u16>(e, "gvec") : nullptr, buf<u16>(e, "y_s"), s);
        scope_set(e);
        FLUXMI_TRY(rc);
      }
    }
    graphs_stale(e, g, rq);
    if (use_graph && !g.ok) {
      if (!g.warmed) {
        if (st.pre_warm) FLUXMI_TRY(st.pre_warm());
        FLUXMI_TRY(pv_eval(e, s, [&]() { return st.step(false); }));
        ++step;
        g.warmed = true;
      }
      if (step < win_end) {
        FLUXMI_CHECK_HIP(hipStreamSynchronize(s));  // one-time, at graph capture only
        FLUXMI_TRY(capture_pieces(g, st.piece, st.n_pieces));
        ++e->captures;
      }
    }
    Range r(st.range);
    // ev_t0 .. ev_t1 (fluxmi_engine_last_timing) brackets frozen STEPS only: recorded behind the first window's modulation table, the eager
    // warm step and the graph capture of a new shape (a request longer than MODS_STEPS steps includes its later table builds)
    if (!t0) {
      FLUXMI_CHECK_HIP(hipEventRecord(e->ev_t0, s));
      *first_timed = step;
      t0 = true;
    }
    const bool graph = use_graph && g.ok;
    int rc = 0;  // (a cancelled call leaves through here as well: what was replayed wrote the buffers)
    for (; step < win_end && !rc; ++step) rc = pv_eval(e, s, [&]() { return st.step(graph); });
    if (graph) {
      // the host code of the step ran at capture only: the replayed pieces wrote the activation buffers in the layout they were captured
      // with (a tuning change since the capture re-captures above)
      const bool ap = act_pairs(e, mode == 1);
      for (bool& b : e->act_in_pairs) b = ap;
    }
    FLUXMI_TRY(rc);
  }
  return 0;
}

// The update of one step, in front of the step counter's advance: the whole stream, or (Kontext) the leading Lpred rows of each sample -- the
// reference rows never move -- or (Fill / Depth / Canny) the leading C_out channels of every row -- the conditioning channels never move (no
// row split then: prepare_cond).  With an inpainting state set (fluxmi_engine_set_inpaint) the ONE blend kernel replaces whichever of them
// it would have been.  With a solver program set (fluxmi_engine_set_solver) the ONE table-driven update replaces all of them, the blend
// included: a step is then one evaluation, and the d_dts table goes unused; a stochastic program runs the kernel's noise form.  Guidance
// shaping: moments and combine on pred_s in front of whichever guided update runs; both halves of pred_s then hold the shaped prediction v,
// and the update's own chain d = bf16(v - v) = 0, m = 0, p = v steps with v unchanged.  The preview launch goes in front of whichever
// update runs, behind the shaping -- both halves of pred_s then hold v, and the guided formula u + s (v - v) still gives v.
int update_launch(E* e, const Request& rq, hipStream_t st) {
  const int B = e->B, Li = e->Li, C = e->d.in_channels, Co = c_out(e);
  u16 *img_s = buf<u16>(e, "img_s"), *pred_s = buf<u16>(e, "pred_s");
  const float* scale = rq.cfg() ? e->d_cfg : nullptr;
  if (rq.win()) {
    const int* g = e->win_geo;
    const char* tab = buf<char>(e, "win_tab");
    return fluxmi_k_window_step(buf<u16>(e, "win_x"), img_s, pred_s, e->d_dts, e->d_step, scale, (const int*)(tab + e->win_off[0]),
                                (const int*)(tab + e->win_off[1]), (const float*)(tab + e->win_off[2]), (const float*)(tab + e->win_off[3]), g[0],
                                g[1], g[2], g[3], g[4], g[5], g[6], C, st);
  }
  if (rq.edit()) {
    const FeTab* tab = buf<FeTab>(e, "fe_tab");
    return fluxmi_k_flowedit_step(img_s, pred_s, buf<u16>(e, "fe_z"), buf<float>(e, "fe_acc"), buf<u16>(e, "fe_x0"), tab->coef, tab->ctl, e->d_step,
                                  tab->draw.ids, &tab->draw.offset, rq.images, Li, e->Lpred, C, Co, st);
  }
  if (rq.shaped) {
    const long long n_pred = (long long)e->Lpred * Co;
    float* gp = buf<float>(e, "gd_params");
    FLUXMI_TRY(fluxmi_k_guidance_moments(pred_s, buf<float>(e, "gd_r"), buf<float>(e, "gd_part"), rq.images, n_pred, st));
    FLUXMI_TRY(fluxmi_k_guidance_combine(pred_s, buf<float>(e, "gd_r"), buf<float>(e, "gd_part"), gp, e->d_step, (const int*)(gp + 8),
                                         buf<float>(e, "gd_coef"), rq.images, n_pred, st));
  }
  if (rq.previewed)
    FLUXMI_TRY(fluxmi_k_latent_preview(img_s, pred_s, e->d_ts, e->d_step, scale, buf<float>(e, "pv_proj"), buf<int>(e, "pv_ctl"),
                                       buf<unsigned char>(e, "pv_out"), rq.images, Li, e->Lpred, C, Co, e->pv_h, e->pv_w, st));
  const u16 *ix0 = e->inp_on ? buf<u16>(e, "inp_x0") : nullptr, *inoise = e->inp_on ? buf<u16>(e, "inp_noise") : nullptr;
  const u16* imask = e->inp_on ? buf<u16>(e, "inp_mask") : nullptr;
  const float* thr = e->inp_on && e->inp_diff ? e->d_thr : nullptr;
  if (rq.sol_noise) {
    const unsigned* ids = buf<unsigned>(e, "sol_ids");
    return fluxmi_k_solver_step_noise(img_s, pred_s, buf<u16>(e, "sol_xs"), buf<float>(e, "sol_hist"), e->d_sol_coef, e->d_sol_ctl, ix0, inoise, imask,
                                      e->d_tnext, e->d_omt, thr, e->d_step, scale, rq.images, Li, e->Lpred, C, Co, ids,
                                      (const int*)(ids + 4 * (size_t)B), st);
  }
  if (e->sol_on)
    return fluxmi_k_solver_step(img_s, pred_s, buf<u16>(e, "sol_xs"), buf<float>(e, "sol_hist"), e->d_sol_coef, e->d_sol_ctl, ix0, inoise, imask,
                                e->d_tnext, e->d_omt, thr, e->d_step, scale, rq.images, Li, e->Lpred, C, Co, st);
  if (e->inp_on)
    return fluxmi_k_blend_euler(img_s, pred_s, ix0, inoise, imask, e->d_dts, e->d_tnext, e->d_omt, thr, e->d_step, scale, rq.images, Li, e->Lpred, C,
                                Co, st);
  if (rq.cfg()) return fluxmi_k_cfg_euler(img_s, pred_s, e->d_dts, e->d_step, e->d_cfg, rq.images, Li, e->Lpred, C, Co, st);
  return fluxmi_k_euler_step("euler", img_s, pred_s, nullptr, nullptr, nullptr, e->d_dts, nullptr, nullptr, nullptr, e->d_step, nullptr, B, Li,
                             e->Lpred, C, Co, st);
}

// The plain step: one piece -- the forward, the update, the step counter -- and one hipGraphLaunch per replayed step.
int plain_steps(E* e, int mode, const Request& rq, int step, const u16* g_arg, int use_graph, int* first_timed) {
  hipStream_t s = rq.s;
  Stepper st;
  st.g = &e->step_graphs;
  st.range = "frozen steps (hipGraph replay)";
  st.n_pieces = 1;
  st.piece[0] = {"the step", [&](hipStream_t t) -> int {
                   FLUXMI_TRY(frozen_forward(e, mode, g_arg, PH_EMBED, PH_FINAL, t));
                   FLUXMI_TRY(update_launch(e, rq, t));
                   return fluxmi_k_advance_step(e->d_step, t);
                 }};
  st.step = [&](bool graph) -> int {
    if (!graph) return st.piece[0].run(s);
    FLUXMI_CHECK_HIP(hipGraphLaunch(st.g->exec[0], s));
    return 0;
  };
  return frozen_steps(e, st, mode, rq, step, g_arg, use_graph, first_timed);
}

// The step with first-block caching (fluxmi.h, fluxmi_engine_set_step_cache): three pieces with a host decision between them
//   head: img_in, txt rows, select_step | h0 = x rows | double block 0 | r = bf16(x - h0) over h0, ratios -> pinned host
//   host: waits for the head, reads the B ratios, decides
//   body (miss): r_ref = r, h1 = x | blocks 1 .. | R = bf16(x - h1) | final layer, update, advance
//   skip (hit):  x = bf16(x + R) (x still holds this step's h1) | final layer, update, advance
// on the rows the final layer reads.  The rule's host state (have_full, consec) and the log live here; a plain request never comes here, so it
// never allocates, captures or launches anything of the cache.
int cached_steps(E* e, int mode, const Request& rq, int step, const u16* g_arg, int use_graph, int* first_timed) {
  hipStream_t s = rq.s;
  FLUXMI_REQUIRE(e->d.depth >= 1, "engine_denoise: step caching needs at least one double block");
  FLUXMI_TRY(ensure_fb(e, s));
  const int B = e->B, H = e->d.hidden;
  const long long XB = (long long)e->L * H, n = (long long)e->Lpred * H;
  u16* xr = buf<u16>(e, "x") + (long long)e->Lt * H;  // the rows the final layer reads: Lpred rows behind the text rows of each sample
  u16 *h0 = buf<u16>(e, "fb_h0"), *h1 = buf<u16>(e, "fb_h1"), *rref = buf<u16>(e, "fb_rref"), *R = buf<u16>(e, "fb_R");
  float *part = buf<float>(e, "fb_part"), *ratio = buf<float>(e, "fb_ratio");
  auto fwd = [&](int p0, int p1, hipStream_t t) -> int { return frozen_forward(e, mode, g_arg, p0, p1, t); };
  auto tail = [&](hipStream_t t) -> int {
    FLUXMI_TRY(fwd(PH_FINAL, PH_FINAL, t));
    FLUXMI_TRY(update_launch(e, rq, t));
    return fluxmi_k_advance_step(e->d_step, t);
  };
  Stepper st;
  st.g = &e->fb_graphs;
  st.range = "frozen steps (step cache)";
  st.n_pieces = 3;
  st.piece[0] = {"step-cache piece 0 (head)", [&](hipStream_t t) -> int {
                   FLUXMI_TRY(fwd(PH_EMBED, PH_EMBED, t));
                   FLUXMI_TRY(fluxmi_k_fb_snapshot(xr, XB, h0, B, n, t));
                   FLUXMI_TRY(fwd(PH_BLOCK0, PH_BLOCK0, t));
                   FLUXMI_TRY(fluxmi_k_fb_metric(xr, XB, h0, h0, rref, part, ratio, ratio + B, B, n, t));
                   FLUXMI_CHECK_HIP(hipMemcpyAsync(e->h_ratio, ratio, (size_t)B * 4, hipMemcpyDeviceToHost, t));
                   return 0;
                 }};
  st.piece[1] = {"step-cache piece 1 (body)", [&](hipStream_t t) -> int {
                   FLUXMI_TRY(fluxmi_k_fb_commit(xr, XB, h0, rref, h1, B, n, t));
                   FLUXMI_TRY(fwd(PH_BLOCKS, PH_BLOCKS, t));
                   FLUXMI_TRY(fluxmi_k_fb_store(xr, XB, h1, R, B, n, t));
                   return tail(t);
                 }};
  st.piece[2] = {"step-cache piece 2 (skip)", [&](hipStream_t t) -> int {
                   FLUXMI_TRY(fluxmi_k_fb_apply(xr, XB, xr, XB, R, B, n, t));
                   return tail(t);
                 }};
  // host state of the rule
  bool have_full = false;  // a full step has run in THIS call: every call starts with an empty cache
  int consec = 0;
  e->fb_log_B = B;
  auto run = [&](int p, bool graph) -> int {
    if (!graph) return st.piece[p].run(s);
    FLUXMI_CHECK_HIP(hipGraphLaunch(st.g->exec[p], s));
    return 0;
  };
  st.step = [&](bool graph) -> int {
    FLUXMI_TRY(run(0, graph));
    FLUXMI_CHECK_HIP(hipEventRecord(e->ev_fb, s));
    FLUXMI_CHECK_HIP(hipEventSynchronize(e->ev_fb));
    bool hit = have_full && (e->fb_max_hits <= 0 || consec < e->fb_max_hits);
    for (int b = 0; b < B; ++b) {
      const float r = have_full ? e->h_ratio[b] : INFINITY;  // no reference yet: the step misses whatever r_ref still holds
      e->fb_log_ratio.push_back(r);
      hit = hit && r < e->fb_threshold;  // NaN and +inf (den == 0) are misses
    }
    e->fb_log_hit.push_back(hit ? 1 : 0);
    consec = hit ? consec + 1 : 0;
    have_full = have_full || !hit;
    return run(hit ? 2 : 1, graph);
  };
  // lazy one-time inits happen outside capture: the warm step runs head and body eagerly -- it is the first frozen step of a call and
  // misses -- and the skip piece's own kernel is launched once before it on x's image rows, which are dead here (img_in rewrites them next)
  st.pre_warm = [&]() -> int {
    FLUXMI_REQUIRE(!have_full, "engine_denoise: step-cache warm-up behind a full step");
    return fluxmi_k_fb_apply(xr, XB, xr, XB, R, B, n, s);
  };
  return frozen_steps(e, st, mode, rq, step, g_arg, use_graph, first_timed);
}

// ---- the phases of a denoise call, in the order denoise_impl runs them ---------------------------------------------------------------------------
int check_call(E* e, const Request& rq, const void* img, const void* txt, const void* y, const double* timesteps_host, const int* trial_index_inout) {
  FLUXMI_REQUIRE(e && e->ws, "engine_denoise: call fluxmi_engine_prepare first");
  FLUXMI_REQUIRE(!e->is_cn, "engine_denoise: a ControlNet engine runs attached to a main engine (fluxmi_engine_attach_controlnet)");
  FLUXMI_REQUIRE(!rq.cfg() || e->B % 2 == 0, "engine_denoise_cfg: the prepared batch (%d) must be even: prompt branches first, then the negative "
                 "branches of the same images (2B <= %d)", e->B, FLUXMI_ENGINE_MAX_BATCH);
  FLUXMI_REQUIRE(img && txt && y && timesteps_host && trial_index_inout, "engine_denoise: NULL argument");
  FLUXMI_REQUIRE(rq.n_steps >= 0 && rq.n_steps <= MAX_STEPS, "engine_denoise: n_steps=%d out of range", rq.n_steps);
  return 0;
}

// what an edit call excludes; it makes the edit state's buffers and marks the running call
int check_edit(E* e, const Request& rq) {
  hipStream_t s = rq.s;
  const int n_steps = rq.n_steps;
  FLUXMI_REQUIRE(e->fe_on, "engine_denoise_edit: no FlowEdit state is set (fluxmi_engine_set_flow_edit)");
  FLUXMI_REQUIRE(e->B % 2 == 0, "engine_denoise_edit: the prepared batch (%d) must be even: source branches first, then the target branches "
                 "of the same images (2B <= %d)", e->B, FLUXMI_ENGINE_MAX_BATCH);
  FLUXMI_REQUIRE(e->Lpred == e->Li && c_out(e) == e->d.in_channels, "engine_denoise_edit: %d reference rows, %d input and %d predicted "
                 "channels: FlowEdit steps the whole stream (no Kontext reference, no Fill / Depth / Canny model)", e->Li - e->Lpred,
                 e->d.in_channels, c_out(e));
  FLUXMI_REQUIRE(e->fe_B == e->B / 2, "engine_denoise_edit: the FlowEdit state holds %d images, this call steps %d (half the prepared batch)",
                 e->fe_B, e->B / 2);
  FLUXMI_REQUIRE(e->fe_n == n_steps, "engine_denoise_edit: the FlowEdit program holds %d evaluations, this call runs %d "
                 "(fluxmi_engine_set_flow_edit takes one row per evaluation of the call)", e->fe_n, n_steps);
  FLUXMI_REQUIRE(!e->inp_on, "engine_denoise_edit: an inpainting state is set (FlowEdit edits the whole image: no mask)");
  FLUXMI_REQUIRE(!e->sol_on, "engine_denoise_edit: a solver program is set (FlowEdit's update is its own: sampler euler only)");
  FLUXMI_REQUIRE(!(e->fb_threshold > 0.f), "engine_denoise_edit: step caching is on (every evaluation runs on a fresh draw: consecutive "
                 "evaluations are not comparable)");
  FLUXMI_REQUIRE(!e->masked, "engine_denoise_edit: an attention-group table is set (regional prompts do not combine with FlowEdit)");
  FLUXMI_REQUIRE(!e->cn, "engine_denoise_edit: a ControlNet is attached (not combined with FlowEdit)");
  FLUXMI_REQUIRE(!e->ip_on, "engine_denoise_edit: an IP-Adapter is set (not combined with FlowEdit)");
  FLUXMI_REQUIRE(!(e->pv_hook && e->pv_every > 0), "engine_denoise_edit: previews (every = %d > 0) are refused: the stream holds the two "
                 "coupled model inputs, not a latent to preview (a hook with every = 0 reports progress and cancels)", e->pv_every);
  FLUXMI_TRY(e->side[SB_FE_Z].ensure(e, {{"fe_z", fe_elems(e) * 2}}, true, s, "engine_flow_edit", " (fe_z)"));
  if (e->fe_need_acc) FLUXMI_TRY(e->side[SB_FE_ACC].ensure(e, {{"fe_acc", fe_elems(e) * 4}}, true, s, "engine_flow_edit", " (fe_acc)"));
  e->fe_call = true;
  return 0;
}

// what a windowed call excludes; it marks the running call
int check_windows(E* e, const Request& rq) {
  const bool cfg = rq.cfg();
  const int *g = e->win_geo, S = g[0] * g[5] * g[6];
  FLUXMI_REQUIRE(e->win_on, "engine_denoise_windows: no window state is set (fluxmi_engine_set_windows)");
  FLUXMI_REQUIRE(e->B == (cfg ? 2 * S : S) && e->Li == g[3] * g[4], "engine_denoise_windows: the window state holds %d images x %d x %d "
                 "windows of %d x %d tokens, the prepared shape %d samples of %d rows (%s: %d samples of %d)", g[0], g[5], g[6], g[3], g[4],
                 e->B, e->Li, cfg ? "guided" : "unguided", cfg ? 2 * S : S, g[3] * g[4]);
  FLUXMI_REQUIRE(e->Lpred == e->Li && c_out(e) == e->d.in_channels, "engine_denoise_windows: %d reference rows, %d input and %d predicted "
                 "channels: a windowed call steps the whole stream (no Kontext reference, no Fill / Depth / Canny model)", e->Li - e->Lpred,
                 e->d.in_channels, c_out(e));
  FLUXMI_REQUIRE(!e->inp_on, "engine_denoise_windows: an inpainting state is set (windows are not combined with a mask)");
  FLUXMI_REQUIRE(!e->sol_on, "engine_denoise_windows: a solver program is set (the windowed update is its own: sampler euler only)");
  FLUXMI_REQUIRE(!(e->fb_threshold > 0.f), "engine_denoise_windows: step caching is on (not combined with windows)");
  FLUXMI_REQUIRE(!e->masked, "engine_denoise_windows: an attention-group table is set (regional prompts do not combine with windows)");
  FLUXMI_REQUIRE(!e->cn, "engine_denoise_windows: a ControlNet is attached (not combined with windows)");
  FLUXMI_REQUIRE(!e->ip_on, "engine_denoise_windows: an IP-Adapter is set (not combined with windows)");
  FLUXMI_REQUIRE(!e->fe_on, "engine_denoise_windows: a FlowEdit state is set (not combined with windows)");
  FLUXMI_REQUIRE(!(cfg && e->gd_on), "engine_denoise_windows: guidance shaping is set (a guided windowed call is unshaped)");
  FLUXMI_REQUIRE(!(e->pv_hook && e->pv_every > 0), "engine_denoise_windows: previews (every = %d > 0) are refused: the stream holds windows, "
                 "not the canvas (a hook with every = 0 reports progress and cancels)", e->pv_every);
  e->win_call = true;
  return 0;
}

// what the feature states set on the engine ask of this call, each followed by the side allocation its first request makes; the hook state
// of the running call starts here
int check_features(E* e, const Request& rq) {
  hipStream_t s = rq.s;
  const int n_steps = rq.n_steps;
  FLUXMI_REQUIRE(!e->inp_on || e->inp_B == rq.images, "engine_denoise: the inpainting state holds %d images, this call steps %d "
                 "(fluxmi_engine_set_inpaint takes the caller's images: the prepared batch, half of it for a guided call)", e->inp_B, rq.images);
  FLUXMI_REQUIRE(!e->inp_on || !e->inp_diff || (int)e->inp_thr.size() == n_steps, "engine_denoise: %d differential thresholds for a call of %d "
                 "steps (fluxmi_engine_set_inpaint takes one per step)", (int)e->inp_thr.size(), n_steps);
  FLUXMI_REQUIRE(!e->sol_on || e->sol_n == n_steps, "engine_denoise: the solver program holds %d evaluations, this call runs %d "
                 "(fluxmi_engine_set_solver takes one row per step of the call)", e->sol_n, n_steps);
  FLUXMI_REQUIRE(!e->sol_on || !(e->fb_threshold > 0.f), "engine_denoise: a solver program does not combine with step caching (the cache "
                 "compares consecutive evaluations; a solver may evaluate one time twice)");
  // A stochastic program (a non-zero cn in column 7) needs its ids (fluxmi_engine_set_solver_noise)
  bool sol_cn = false;
  for (int i = 0; e->sol_on && i < n_steps; ++i) sol_cn = sol_cn || e->sol_coef[(size_t)8 * i + 7] != 0.f;
  FLUXMI_REQUIRE(!sol_cn || e->sol_noise, "engine_denoise: the solver program has a non-zero noise coefficient and no ids are set "
                 "(fluxmi_engine_set_solver_noise after fluxmi_engine_set_solver)");
  FLUXMI_REQUIRE(!rq.sol_noise || e->sol_noise_B == rq.images, "engine_denoise: the solver noise holds ids of %d images, this call steps %d "
                 "(fluxmi_engine_set_solver_noise takes the caller's images: the prepared batch, half of it for a guided call)", e->sol_noise_B,
                 rq.images);
  if (e->sol_on) FLUXMI_TRY(ensure_sol(e, s));
  if (rq.sol_noise)  // the device copy of the noise ids and the evaluation offset; not zeroed: every call stages it
    FLUXMI_TRY(e->side[SB_SOL_IDS].ensure(e, {{"sol_ids", up256((size_t)e->B * 16 + 4)}}, false, s, "engine_denoise", " (solver noise ids)"));
  if (rq.shaped) {  // the guidance-shaping buffers of the prepared shape, for the caller's Bh images
    const size_t Bh = rq.images, n = (size_t)e->Lpred * c_out(e), chunks = (n + GD_CHUNK_ELEMS - 1) / GD_CHUNK_ELEMS;
    FLUXMI_TRY(e->side[SB_GD].ensure(e, {{"gd_params", 9 * 4}, {"gd_part", Bh * chunks * 9 * 4}, {"gd_coef", Bh * 4 * 4}, {"gd_r", Bh * n * 4}}, true, s,
                                     "engine_denoise", " (guidance shaping)"));
  }
  FLUXMI_REQUIRE(!rq.hooked || !e->amax_hook, "engine_denoise: a step hook and an amax-exchange hook are both set (previews, progress and "
                 "cancellation are refused under a process group: the host waits would stall its collectives)");
  FLUXMI_REQUIRE(!rq.previewed || ((long long)e->pv_h * e->pv_w == e->Lpred && c_out(e) == 64), "engine_denoise: the preview state's token grid "
                 "%d x %d does not cover the %d stepped rows of the prepared shape (or C_out = %d != 64)", e->pv_h, e->pv_w, e->Lpred, c_out(e));
  if (rq.previewed)  // the preview buffers of the prepared shape: room for a plain call's B images
    FLUXMI_TRY(e->side[SB_PV].ensure(e, {{"pv_proj", 51 * 4}, {"pv_ctl", 2 * 4}, {"pv_out", (size_t)FLUXMI_PREVIEW_SLOTS * e->B * e->Lpred * 4 * 3}},
                                     true, s, "engine_denoise", " (preview)"));
  e->pv_launched = e->pv_delivered = 0;
  e->pv_cancelled = false;
  e->pv_images = rq.win() ? e->win_geo[0] : rq.images;
  if (e->ip_on) FLUXMI_TRY(ip_usable(e));
  // the attached ControlNet: its own scratch / weight copies, the request's schedule and step counter shared with the main engine
  if (e->cn) {
    FLUXMI_TRY(cn_usable(e));
    FLUXMI_REQUIRE(e->cn_batch == rq.images, "engine_denoise: the attached ControlNet's cond holds %d images, this call steps %d", e->cn_batch,
                   rq.images);
    FLUXMI_TRY(ensure_pairs(e->cn, s));
  }
  return 0;
}

// The call's tables -> device through the engine's pinned staging buffer.  The buffer may still be the source of the previous request's
// (long finished) copy: wait on that copy's event, never on the stream.
int stage_tables(E* e, const Request& rq, const double* timesteps_host) {
  hipStream_t s = rq.s;
  const int n_steps = rq.n_steps, B = e->B;
  const bool edit = rq.edit();
  if (e->sched_pending) FLUXMI_CHECK_HIP(hipEventSynchronize(e->ev_sched));
  SchedStaging* h = e->h_sched;
  // (an edit call: timesteps_host holds the n_steps evaluation times and nothing behind them; the dts table goes unused)
  for (int i = 0; i <= n_steps; ++i) h->ts[i] = edit && i == n_steps ? 0.f : (float)timesteps_host[i];
  for (int i = 0; i < n_steps; ++i) h->dts[i] = edit ? 0.f : (float)(timesteps_host[i + 1] - timesteps_host[i]);
  h->dts[n_steps] = 0.f;
  FLUXMI_CHECK_HIP(hipMemcpyAsync(e->d_ts, h->ts, (n_steps + 1) * 4, hipMemcpyHostToDevice, s));
  FLUXMI_CHECK_HIP(hipMemcpyAsync(e->d_dts, h->dts, (n_steps + 1) * 4, hipMemcpyHostToDevice, s));
  if (e->inp_on) {  // the blend's tables: the NEXT time of every step and its complement (subtracted in double), the thresholds
    for (int i = 0; i < n_steps; ++i) {
      h->tnext[i] = (float)timesteps_host[i + 1];
      h->omt[i] = (float)(1.0 - timesteps_host[i + 1]);
      h->thr[i] = e->inp_diff ? (float)e->inp_thr[i] : 0.f;
    }
    h->tnext[n_steps] = h->omt[n_steps] = h->thr[n_steps] = 0.f;
    FLUXMI_CHECK_HIP(hipMemcpyAsync(e->d_tnext, h->tnext, (n_steps + 1) * 4, hipMemcpyHostToDevice, s));
    FLUXMI_CHECK_HIP(hipMemcpyAsync(e->d_omt, h->omt, (n_steps + 1) * 4, hipMemcpyHostToDevice, s));
    if (e->inp_diff) FLUXMI_CHECK_HIP(hipMemcpyAsync(e->d_thr, h->thr, (n_steps + 1) * 4, hipMemcpyHostToDevice, s));
  }
  if (e->sol_on && n_steps > 0) {  // the solver's tables, through the same staging buffer
    memcpy(h->sol_coef, e->sol_coef.data(), (size_t)n_steps * 8 * 4);
    memcpy(h->sol_ctl, e->sol_ctl.data(), (size_t)n_steps * 4 * 4);
    FLUXMI_CHECK_HIP(hipMemcpyAsync(e->d_sol_coef, h->sol_coef, (size_t)n_steps * 8 * 4, hipMemcpyHostToDevice, s));
    FLUXMI_CHECK_HIP(hipMemcpyAsync(e->d_sol_ctl, h->sol_ctl, (size_t)n_steps * 4 * 4, hipMemcpyHostToDevice, s));
  }
  if (rq.sol_noise) {  // ... and the noise ids with the evaluation offset behind them (one copy: the offset sits at [B][4] of "sol_ids")
    memset(h->sol_ids, 0, (size_t)B * 16);
    memcpy(h->sol_ids, e->sol_ids.data(), (size_t)e->sol_noise_B * 16);
    h->sol_ids[4 * (size_t)B] = (unsigned)e->sol_eval_offset;
    FLUXMI_CHECK_HIP(hipMemcpyAsync(buf<unsigned>(e, "sol_ids"), h->sol_ids, (size_t)B * 16 + 4, hipMemcpyHostToDevice, s));
  }
  if (rq.shaped) {  // ... and the shaping parameters with the step offset behind them; a new request's running difference starts at 0
    memcpy(h->gd.params, e->gd_params, 32);
    h->gd.offset = e->gd_offset;
    FLUXMI_CHECK_HIP(hipMemcpyAsync(buf<float>(e, "gd_params"), &h->gd, 36, hipMemcpyHostToDevice, s));
    if (e->gd_zero_r) FLUXMI_CHECK_HIP(hipMemsetAsync(buf<float>(e, "gd_r"), 0, (size_t)rq.images * e->Lpred * c_out(e) * 4, s));
    e->gd_zero_r = false;
  }
  if (rq.previewed) {  // ... and the projection, and the control word {every, eval_offset}
    memcpy(h->pv.proj, e->pv_proj, 51 * 4);
    h->pv.ctl[0] = e->pv_every;
    h->pv.ctl[1] = e->pv_offset;
    FLUXMI_CHECK_HIP(hipMemcpyAsync(buf<float>(e, "pv_proj"), h->pv.proj, 51 * 4, hipMemcpyHostToDevice, s));
    FLUXMI_CHECK_HIP(hipMemcpyAsync(buf<int>(e, "pv_ctl"), h->pv.ctl, 8, hipMemcpyHostToDevice, s));
  }
  if (edit) {  // ... and FlowEdit's tables, ids and offset: one copy each into "fe_tab"
    FeTab* tab = buf<FeTab>(e, "fe_tab");
    memcpy(h->fe.coef, e->fe_coef.data(), (size_t)n_steps * 16);
    memcpy(h->fe.ctl, e->fe_ctl.data(), (size_t)n_steps * 8);
    memset(h->fe.draw.ids, 0, sizeof h->fe.draw.ids);
    memcpy(h->fe.draw.ids, e->fe_ids.data(), (size_t)e->fe_B * 16);
    h->fe.draw.offset = e->fe_eval_offset;
    if (n_steps > 0) {
      FLUXMI_CHECK_HIP(hipMemcpyAsync(tab->coef, h->fe.coef, (size_t)n_steps * 16, hipMemcpyHostToDevice, s));
      FLUXMI_CHECK_HIP(hipMemcpyAsync(tab->ctl, h->fe.ctl, (size_t)n_steps * 8, hipMemcpyHostToDevice, s));
    }
    FLUXMI_CHECK_HIP(hipMemcpyAsync(&tab->draw, &h->fe.draw, sizeof h->fe.draw, hipMemcpyHostToDevice, s));
  }
  FLUXMI_CHECK_HIP(hipEventRecord(e->ev_sched, s));
  e->sched_pending = true;
  return 0;
}

// elements of the caller's latent: the canvas of a windowed call, else the caller's samples
long long caller_elems(const E* e, const Request& rq) {
  return rq.win() ? (long long)e->win_geo[0] * e->win_geo[1] * e->win_geo[2] * e->d.in_channels : (long long)rq.images * e->Li * e->d.in_channels;
}

// The caller's inputs -> the engine's static request buffers, on the stream: the guidance vector, the step counter, the latent (canvas
// gather, edit coupling, or the copy or copies), the guidance scale, text and y.
int load_inputs(E* e, const Request& rq, const void* img, const void* txt, const void* y, const double* timesteps_host) {
  hipStream_t s = rq.s;
  const int B = e->B, Li = e->Li, C = e->d.in_channels;
  u16 *gvec = buf<u16>(e, "gvec"), *img_s = buf<u16>(e, "img_s");
  if (rq.edit()) {  // a distilled-guidance value per branch: the source half, then the target half
    FLUXMI_TRY(fluxmi_k_fill_bf16(gvec, e->fe_gs, B / 2, s));
    FLUXMI_TRY(fluxmi_k_fill_bf16(gvec + B / 2, e->fe_gt, B / 2, s));
  } else {
    FLUXMI_TRY(fluxmi_k_fill_bf16(gvec, rq.guidance, B, s));  // guidance arrives in the flow dtype (flux_pipeline.py:619-623)
  }
  FLUXMI_CHECK_HIP(hipMemsetAsync(e->d_step, 0, 4, s));
  const long long n_img = caller_elems(e, rq);
  if (rq.win()) {  // the caller's canvas goes beside the stream; one gather fills every window of it (guided: both halves)
    const int* g = e->win_geo;
    const char* tab = buf<char>(e, "win_tab");
    u16* wx = buf<u16>(e, "win_x");
    FLUXMI_CHECK_HIP(hipMemcpyAsync(wx, img, n_img * 2, hipMemcpyDeviceToDevice, s));
    FLUXMI_TRY(fluxmi_k_window_gather(wx, img_s, (const int*)(tab + e->win_off[0]), (const int*)(tab + e->win_off[1]), g[0], g[1], g[2], g[3],
                                      g[4], g[5], g[6], C, rq.cfg() ? 1 : 0, s));
  } else if (rq.edit()) {  // the caller's edit state goes beside the stream; the first coupling, at the first evaluation's time, fills both halves of it
    u16* fz = buf<u16>(e, "fe_z");
    FLUXMI_CHECK_HIP(hipMemcpyAsync(fz, img, n_img * 2, hipMemcpyDeviceToDevice, s));
    if (rq.n_steps > 0)
      FLUXMI_TRY(fluxmi_k_flowedit_couple(img_s, fz, buf<u16>(e, "fe_x0"), (float)timesteps_host[0], (float)(1.0 - timesteps_host[0]),
                                          buf<FeTab>(e, "fe_tab")->draw.ids, (unsigned)e->fe_eval_offset, B / 2, Li, e->Lpred, C, c_out(e), s));
  } else {
    FLUXMI_CHECK_HIP(hipMemcpyAsync(img_s, img, n_img * 2, hipMemcpyDeviceToDevice, s));
  }
  if (rq.cfg()) {
    if (!rq.win()) FLUXMI_CHECK_HIP(hipMemcpyAsync(img_s + n_img, img, n_img * 2, hipMemcpyDeviceToDevice, s));
    unsigned bits;
    memcpy(&bits, &rq.cfg_scale, 4);
    FLUXMI_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)e->d_cfg, (int)bits, 1, s));
  }
  FLUXMI_CHECK_HIP(hipMemcpyAsync(buf<u16>(e, "txt_s"), txt, (size_t)B * e->Lt * e->d.ctx_in * 2, hipMemcpyDeviceToDevice, s));
  FLUXMI_CHECK_HIP(hipMemcpyAsync(buf<u16>(e, "y_s"), y, (size_t)B * e->d.vec_in * 2, hipMemcpyDeviceToDevice, s));
  return 0;
}

// The calibrating steps: the reference's first num_trials + 1 calls of every F8Linear, unfused.  With a ControlNet attached: while EITHER
// net has trials left -- that net in mode 0, the other in its frozen mode, eagerly.  Advances *trial and *step; a cancelled call leaves
// through here with pv_cancelled set.
int calibrating_steps(E* e, const Request& rq, const u16* g_arg, int* trial, int* step) {
  Range r("calibrating steps (unfused)");
  hipStream_t s = rq.s;
  E* const cn = e->cn;
  const bool main_f8 = any_f8(e), cn_f8 = cn && any_f8(cn);
  u16 *gvec = buf<u16>(e, "gvec"), *tvec = buf<u16>(e, "tvec");
  u16 *img_s = buf<u16>(e, "img_s"), *txt_s = buf<u16>(e, "txt_s"), *y_s = buf<u16>(e, "y_s"), *pred_s = buf<u16>(e, "pred_s");
  auto main_cal = [&]() { return main_f8 && *trial <= e->d.num_trials; };
  auto cn_cal = [&]() { return cn_f8 && cn->cn_trial <= cn->d.num_trials; };
  auto cal_step = [&]() -> int {
    FLUXMI_TRY(fluxmi_k_set_timestep(tvec, e->d_ts, e->d_step, e->B, s));
    if (cn) {
      const int nmode = cn_cal() ? 0 : (all_block_linears_f8(cn) ? 1 : 2);
      if (nmode == 0) cn->qlut_valid = false;
      if (nmode == 1) FLUXMI_TRY(build_qluts(cn, s));
      FLUXMI_TRY(cn_forward(e, img_s, txt_s, y_s, tvec, gvec, nmode, cn->cn_trial, false, s));
      if (nmode == 0) ++cn->cn_trial;
    }
    const int mmode = main_cal() ? 0 : (all_block_linears_f8(e) ? 1 : 2);
    if (mmode == 0) e->qlut_valid = false;
    if (mmode == 1) FLUXMI_TRY(build_qluts(e, s));
    FLUXMI_TRY(forward_impl(e, img_s, txt_s, y_s, tvec, g_arg, pred_s, mmode, *trial, false, s));
    FLUXMI_TRY(update_launch(e, rq, s));
    FLUXMI_TRY(fluxmi_k_advance_step(e->d_step, s));
    if (mmode == 0) ++*trial;
    ++*step;
    return 0;
  };
  while (*step < rq.n_steps && (main_cal() || cn_cal())) {
    const int rc = pv_eval(e, s, cal_step);
    if (rc == FLUXMI_CANCELLED && e->pv_cancelled) break;
    FLUXMI_TRY(rc);
  }
  return 0;
}

// The frozen steps [step, n_steps): the embedded text and the quantising tables once per request, then the plain loop or the one with
// first-block step caching (the same steps cut into head / body / skip pieces with a host decision in between).
int frozen_part(E* e, const Request& rq, const u16* g_arg, int step, int use_graph) {
  hipStream_t s = rq.s;
  E* const cn = e->cn;
  const int n_steps = rq.n_steps;
  u16* txt_s = buf<u16>(e, "txt_s");
  e->timed_steps = 0;
  e->fb_log_ratio.clear();
  e->fb_log_hit.clear();
  if (step >= n_steps || e->pv_cancelled) return 0;
  const int mode = all_block_linears_f8(e) ? 1 : 2;  // any bf16 block linear -> the fused path is unavailable, run unfused-frozen
  if (mode == 1) {
    FLUXMI_TRY(embed_txt(e, txt_s, false, 0, buf<u16>(e, "txt_emb"), (long long)e->Lt * e->d.hidden, s));
    e->txt_emb_valid = true;
    FLUXMI_TRY(build_qluts(e, s));
  }
  if (cn && all_block_linears_f8(cn)) {  // the net's embedded text (behind its mode row) and quantising tables, once per request
    scope_set(cn);
    u16* te = buf<u16>(cn, "txt_emb");
    int rc = embed_txt(cn, txt_s, false, 0, te, (long long)cn->Lt * cn->d.hidden, s);
    if (!rc) rc = put_mode_row(cn, te, (long long)cn->Lt * cn->d.hidden, s);
    if (!rc) rc = build_qluts(cn, s);
    scope_set(e);
    FLUXMI_TRY(rc);
    cn->txt_emb_valid = true;
  }
  int first_timed = n_steps;  // the first step behind ev_t0, which the loop records: ev_t0 .. ev_t1 brackets steps [first_timed, n_steps)
  const int rc = (e->fb_threshold > 0.f ? cached_steps : plain_steps)(e, mode, rq, step, g_arg, use_graph, &first_timed);
  if (!(rc == FLUXMI_CANCELLED && e->pv_cancelled)) FLUXMI_TRY(rc);
  FLUXMI_CHECK_HIP(hipEventRecord(e->ev_t1, s));
  e->timed_steps = e->pv_cancelled ? std::max(0, e->pv_launched - first_timed) : n_steps - first_timed;
  return 0;
}

// A hooked call drains: the evaluations still in flight are waited for and delivered, so the call is synchronous.  A cancelled one delivers
// nothing further and waits for what it launched.  Then the latent goes back to the caller.
int drain_and_copy_back(E* e, const Request& rq, void* img) {
  while (rq.hooked && !e->pv_cancelled && e->pv_delivered < e->pv_launched) FLUXMI_TRY(pv_deliver(e, e->pv_delivered));
  if (e->pv_cancelled && e->pv_launched > 0)
    FLUXMI_CHECK_HIP(hipEventSynchronize(e->pv_ev[(e->pv_launched - 1) % (FLUXMI_PREVIEW_DEPTH + 1)]));
  const u16* src = rq.win() ? buf<u16>(e, "win_x") : (rq.edit() ? buf<u16>(e, "fe_z") : buf<u16>(e, "img_s"));
  FLUXMI_CHECK_HIP(hipMemcpyAsync(img, src, caller_elems(e, rq) * 2, hipMemcpyDeviceToDevice, rq.s));
  return 0;
}

// the denoise loop of every kind of request
int denoise_impl(E* e, const Request& rq, void* img, const void* txt, const void* y, const double* timesteps_host, int* trial_index_inout,
                 int use_graph) {
  if (e) e->fe_call = e->win_call = false;
  FLUXMI_TRY(check_call(e, rq, img, txt, y, timesteps_host, trial_index_inout));
  if (rq.edit()) FLUXMI_TRY(check_edit(e, rq));
  if (rq.win()) FLUXMI_TRY(check_windows(e, rq));
  struct EditCallScope {  // fe_call and win_call speak of the running call only: off again on every way out
    E* e;
    ~EditCallScope() { e->fe_call = e->win_call = false; }
  } edit_scope{e};
  Range whole("fluxmi_engine_denoise");
  SplitkScope splitk(e);
  FLUXMI_TRY(ensure_pairs(e, rq.s));
  FLUXMI_TRY(check_features(e, rq));
  // for the length of this call the attached ControlNet reads the request's schedule and step counter from the main engine's constants; its
  // own pointers are back on every way out
  struct SharedSchedule {
    E* n;
    float* ts;
    int* step;
    SharedSchedule(E* n_, E* m) : n(n_), ts(n_ ? n_->d_ts : nullptr), step(n_ ? n_->d_step : nullptr) {
      if (n) { n->d_ts = m->d_ts; n->d_step = m->d_step; }
    }
    ~SharedSchedule() {
      if (n) { n->d_ts = ts; n->d_step = step; }
    }
  } shared_schedule(e->cn, e);
  FLUXMI_TRY(stage_tables(e, rq, timesteps_host));
  FLUXMI_TRY(load_inputs(e, rq, img, txt, y, timesteps_host));
  int trial = *trial_index_inout, step = 0;
  const u16* g_arg = e->d.guidance_embed ? buf<u16>(e, "gvec") : nullptr;
  FLUXMI_TRY(calibrating_steps(e, rq, g_arg, &trial, &step));
  FLUXMI_TRY(frozen_part(e, rq, g_arg, step, use_graph));
  FLUXMI_TRY(drain_and_copy_back(e, rq, img));
  *trial_index_inout = trial;
  if (e->pv_cancelled) {
    fluxmi_set_error("engine_denoise: cancelled by the step hook after %d of %d evaluations", e->pv_launched, rq.n_steps);
    return FLUXMI_CANCELLED;
  }
  return 0;
}

}  // namespace

extern "C" {

int fluxmi_engine_denoise(fluxmi_engine_t* e, void* img, const void* txt, const void* y, float guidance,
                          const double* timesteps_host, int n_steps, int* trial_index_inout, int use_graph, void* stream) {
  return denoise_impl(e, make_request(e, RQ_PLAIN, guidance, 1.f, n_steps, stream), img, txt, y, timesteps_host, trial_index_inout, use_graph);
}

int fluxmi_engine_denoise_cfg(fluxmi_engine_t* e, void* img, const void* txt, const void* y, float guidance, float cfg_scale,
                              const double* timesteps_host, int n_steps, int* trial_index_inout, int use_graph, void* stream) {
  return denoise_impl(e, make_request(e, RQ_GUIDED, guidance, cfg_scale, n_steps, stream), img, txt, y, timesteps_host, trial_index_inout, use_graph);
}

int fluxmi_engine_denoise_edit(fluxmi_engine_t* e, void* z, const void* txt, const void* y, const double* timesteps_host, int n_evals,
                               int* trial_index_inout, int use_graph, void* stream) {
  return denoise_impl(e, make_request(e, RQ_EDIT, 0.f, 1.f, n_evals, stream), z, txt, y, timesteps_host, trial_index_inout, use_graph);
}

int fluxmi_engine_denoise_windows(fluxmi_engine_t* e, void* canvas, const void* txt, const void* y, float guidance, int guided, float cfg_scale,
                                  const double* timesteps_host, int n_steps, int* trial_index_inout, int use_graph, void* stream) {
  return denoise_impl(e, make_request(e, guided ? RQ_WINDOWED_GUIDED : RQ_WINDOWED, guidance, cfg_scale, n_steps, stream), canvas, txt, y,
                      timesteps_host, trial_index_inout, use_graph);
}

// The window state of the following windowed calls (fluxmi.h): the geometry, and the four host tables copied into the engine's own buffer
// on `stream` (the call returns behind one stream synchronisation: the host tables are the caller's).
int fluxmi_engine_set_windows(fluxmi_engine_t* e, int n_images, int Hc, int Wc, int h, int w, int ny, int nx, const int* row0_host,
                              const int* col0_host, const float* Ny_host, const float* Nx_host, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  FLUXMI_REQUIRE(e, "engine_set_windows: NULL engine");
  if (!row0_host) {
    e->win_on = false;
    return 0;
  }
  FLUXMI_REQUIRE(!e->is_cn, "engine_set_windows: a ControlNet engine steps nothing (set the state on the main engine)");
  FLUXMI_REQUIRE(e->ws, "engine_set_windows: call fluxmi_engine_prepare first (the state belongs to the prepared shape)");
  FLUXMI_REQUIRE(col0_host && Ny_host && Nx_host, "engine_set_windows: row0_host, col0_host, Ny_host and Nx_host go together");
  FLUXMI_REQUIRE(n_images >= 1 && Hc >= 1 && Wc >= 1 && h >= 1 && w >= 1 && ny >= 1 && nx >= 1 && h <= Hc && w <= Wc,
                 "engine_set_windows: bad geometry: %d images, canvas %d x %d, windows %d x %d on a %d x %d grid", n_images, Hc, Wc, h, w, ny, nx);
  FLUXMI_REQUIRE((long long)n_images * ny * nx <= FLUXMI_ENGINE_MAX_BATCH && (long long)n_images * ny * nx <= e->B,
                 "engine_set_windows: %d images x %d x %d windows do not fit the prepared batch of %d samples (one pass: at most %d, half of it "
                 "for a guided call)", n_images, ny, nx, e->B, FLUXMI_ENGINE_MAX_BATCH);
  FLUXMI_REQUIRE(h * w == e->Li, "engine_set_windows: a window of %d x %d tokens is not the prepared shape's %d image rows", h, w, e->Li);
  FLUXMI_REQUIRE((double)n_images * Hc * Wc * (c_out(e) / 8) <= 2147483647.0, "engine_set_windows: the canvas exceeds the kernel's 32-bit index");
  FLUXMI_TRY(fluxmi_window_check_tables("engine_set_windows", row0_host, col0_host, Hc, Wc, h, w, ny, nx));
  for (long long i = 0; i < (long long)ny * Hc; ++i)
    FLUXMI_REQUIRE(std::isfinite(Ny_host[i]), "engine_set_windows: Ny[%lld][%lld] is not finite", i / Hc, i % Hc);
  for (long long i = 0; i < (long long)nx * Wc; ++i)
    FLUXMI_REQUIRE(std::isfinite(Nx_host[i]), "engine_set_windows: Nx[%lld][%lld] is not finite", i / Wc, i % Wc);
  const size_t x_bytes = (size_t)n_images * Hc * Wc * c_out(e) * 2;
  const size_t sz[4] = {(size_t)ny * 4, (size_t)nx * 4, (size_t)ny * Hc * 4, (size_t)nx * Wc * 4};
  size_t off[4], tab_bytes = 0;
  for (int i = 0; i < 4; ++i) { off[i] = tab_bytes; tab_bytes += up256(sz[i]); }
  SideBuf& mem = e->side[SB_WIN];
  if (mem.p && mem.bytes != up256(x_bytes) + tab_bytes) {  // another geometry: pieces captured on the old canvas go stale by the key (graphs_stale)
    FLUXMI_CHECK_HIP(hipStreamSynchronize(s));
    mem.drop(e);
    e->win_on = false;
  }
  FLUXMI_TRY(mem.ensure(e, {{"win_x", x_bytes}, {"win_tab", tab_bytes}}, true, s, "engine_set_windows", " (win_x)"));
  char* tab = buf<char>(e, "win_tab");
  const void* src[4] = {row0_host, col0_host, Ny_host, Nx_host};
  for (int i = 0; i < 4; ++i) FLUXMI_CHECK_HIP(hipMemcpyAsync(tab + off[i], src[i], sz[i], hipMemcpyHostToDevice, s));
  FLUXMI_CHECK_HIP(hipStreamSynchronize(s));
  const int geo[7] = {n_images, Hc, Wc, h, w, ny, nx};
  memcpy(e->win_geo, geo, sizeof geo);
  memcpy(e->win_off, off, sizeof off);
  e->win_on = true;
  return 0;
}

// The FlowEdit state of the following edit calls (fluxmi.h): host tables like the solver program's; x0 is copied into the engine's own buffer
// on `stream`, in order with the denoise_edit call that follows on it.
int fluxmi_engine_set_flow_edit(fluxmi_engine_t* e, const void* x0_dev, int batch, const double* coef_host, const int* ctl_host, int n,
                                const unsigned* ids_host, int eval_offset, float source_guidance, float target_guidance, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  FLUXMI_REQUIRE(e, "engine_set_flow_edit: NULL engine");
  if (!x0_dev) {
    e->fe_on = false;
    e->fe_n = 0;
    e->fe_coef.clear();
    e->fe_ctl.clear();
    e->fe_ids.clear();
    return 0;
  }
  FLUXMI_REQUIRE(!e->is_cn, "engine_set_flow_edit: a ControlNet engine steps nothing (set the state on the main engine)");
  FLUXMI_REQUIRE(e->ws, "engine_set_flow_edit: call fluxmi_engine_prepare first (the state belongs to the prepared shape)");
  FLUXMI_REQUIRE(coef_host && ctl_host && ids_host, "engine_set_flow_edit: x0, coef_host, ctl_host and ids_host go together");
  FLUXMI_REQUIRE(n >= 0 && n <= MAX_STEPS, "engine_set_flow_edit: n=%d out of range (at most %d evaluations)", n, MAX_STEPS);
  FLUXMI_REQUIRE(batch >= 1 && 2 * batch <= std::max(2, e->B), "engine_set_flow_edit: batch %d outside 1..%d (half the prepared batch: "
                 "the source and the target branch of every image)", batch, std::max(1, e->B / 2));
  FLUXMI_REQUIRE(eval_offset >= 0, "engine_set_flow_edit: eval_offset %d < 0", eval_offset);
  FLUXMI_REQUIRE(std::isfinite(source_guidance) && std::isfinite(target_guidance), "engine_set_flow_edit: guidance values must be finite");
  for (int i = 0; i < 4 * n; ++i)
    FLUXMI_REQUIRE(std::isfinite((float)coef_host[i]), "engine_set_flow_edit: coefficient %d of row %d is not finite in fp32", i % 4, i / 4);
  bool need_acc = false;
  for (int i = 0; i < n; ++i) need_acc = need_acc || !ctl_host[2 * i] || !ctl_host[2 * i + 1];
  FLUXMI_TRY(e->side[SB_FE].ensure(e, {{"fe_x0", fe_elems(e) * 2}, {"fe_tab", FE_TAB_BYTES}}, true, s, "engine_flow_edit", " (fe_x0)"));
  FLUXMI_CHECK_HIP(hipMemcpyAsync(buf<void>(e, "fe_x0"), x0_dev, (size_t)batch * e->Lpred * c_out(e) * 2, hipMemcpyDeviceToDevice, s));
  e->fe_coef.resize((size_t)4 * n);
  for (int i = 0; i < 4 * n; ++i) e->fe_coef[i] = (float)coef_host[i];
  e->fe_ctl.resize((size_t)2 * n);
  for (int i = 0; i < 2 * n; ++i) e->fe_ctl[i] = ctl_host[i] != 0;
  e->fe_ids.assign(ids_host, ids_host + 4 * (size_t)batch);
  e->fe_B = batch;
  e->fe_n = n;
  e->fe_eval_offset = eval_offset;
  e->fe_gs = source_guidance;
  e->fe_gt = target_guidance;
  e->fe_need_acc = need_acc;
  e->fe_on = true;
  return 0;
}

// Token-group attention mask of the prepared shape: `table` = [B, L] descriptors on the device (L = Lt + Li: text rows, then image rows, as
// the joint sequence is laid out), copied into the engine's own buffer; NULL = dense.  Self-admission is checked here on a host copy (one
// stream synchronisation per call, none per step).
int fluxmi_engine_set_attn_groups(fluxmi_engine_t* e, const unsigned* table, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  FLUXMI_REQUIRE(e, "engine_set_attn_groups: NULL engine");
  if (!table) {
    e->masked = false;
    return 0;
  }
  FLUXMI_REQUIRE(e->ws, "engine_set_attn_groups: call fluxmi_engine_prepare first (the table is [B, L] of the prepared shape)");
  const size_t n = (size_t)e->B * e->L;
  std::vector<unsigned> h(n);
  FLUXMI_CHECK_HIP(hipMemcpyAsync(h.data(), table, n * 4, hipMemcpyDeviceToHost, s));
  FLUXMI_CHECK_HIP(hipStreamSynchronize(s));
  for (size_t i = 0; i < n; ++i) {
    FLUXMI_REQUIRE((h[i] & 0xFFF0u) == 0, "engine_set_attn_groups: descriptor %zu = 0x%08x has bits 4-15 set", i, h[i]);
    FLUXMI_REQUIRE((h[i] >> (16 + (h[i] & 15u))) & 1u, "engine_set_attn_groups: token %zu (sample %zu, row %zu) does not admit its own key group %u: "
                   "its softmax row would be empty", i, i / e->L, i % e->L, h[i] & 15u);
  }
  FLUXMI_CHECK_HIP(hipMemcpyAsync(buf<unsigned>(e, "attn_groups"), table, n * 4, hipMemcpyDeviceToDevice, s));
  e->masked = true;
  return 0;
}

// Masked-latent inpainting state of the prepared shape (fluxmi.h): the caller's tensors are copied into the engine's own buffers on `stream`,
// in order with the denoise call that follows on it.
int fluxmi_engine_set_inpaint(fluxmi_engine_t* e, const void* x0, const void* noise, const void* mask, int batch, const double* thresholds_host,
                              int n_thresholds, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  FLUXMI_REQUIRE(e, "engine_set_inpaint: NULL engine");
  if (!x0) {
    e->inp_on = e->inp_diff = false;
    e->inp_thr.clear();
    return 0;
  }
  FLUXMI_REQUIRE(e->ws, "engine_set_inpaint: call fluxmi_engine_prepare first (the tensors are [batch, Li, C_out] of the prepared shape)");
  FLUXMI_REQUIRE(noise && mask, "engine_set_inpaint: x0, noise and mask go together");
  FLUXMI_REQUIRE(batch >= 1 && batch <= e->B, "engine_set_inpaint: batch %d outside 1..%d (the prepared batch)", batch, e->B);
  FLUXMI_REQUIRE(!thresholds_host ? n_thresholds == 0 : (n_thresholds >= 0 && n_thresholds <= MAX_STEPS),
                 "engine_set_inpaint: n_thresholds %d (0 without a table, at most %d with one)", n_thresholds, MAX_STEPS);
  for (int i = 0; i < n_thresholds; ++i)
    FLUXMI_REQUIRE(thresholds_host[i] == thresholds_host[i], "engine_set_inpaint: threshold %d is NaN", i);
  const size_t one = up256((size_t)e->B * e->Lpred * c_out(e) * 2);  // (not zeroed: the copies below fill what a call reads)
  FLUXMI_TRY(e->side[SB_INP].ensure(e, {{"inp_x0", one}, {"inp_noise", one}, {"inp_mask", one}}, false, s, "engine_set_inpaint", ""));
  const size_t bytes = (size_t)batch * e->Lpred * c_out(e) * 2;
  FLUXMI_CHECK_HIP(hipMemcpyAsync(buf<void>(e, "inp_x0"), x0, bytes, hipMemcpyDeviceToDevice, s));
  FLUXMI_CHECK_HIP(hipMemcpyAsync(buf<void>(e, "inp_noise"), noise, bytes, hipMemcpyDeviceToDevice, s));
  FLUXMI_CHECK_HIP(hipMemcpyAsync(buf<void>(e, "inp_mask"), mask, bytes, hipMemcpyDeviceToDevice, s));
  e->inp_on = true;
  e->inp_diff = thresholds_host != nullptr;
  e->inp_B = batch;
  e->inp_thr.assign(thresholds_host, thresholds_host + (thresholds_host ? n_thresholds : 0));
  return 0;
}

// The solver program of the following denoise calls (fluxmi.h): host tables only -- the buffers are made by the first denoise call that
// needs them, the device copies travel with every call's schedule.
int fluxmi_engine_set_solver(fluxmi_engine_t* e, const double* coef_host, const int* ctl_host, int n) {
  FLUXMI_REQUIRE(e, "engine_set_solver: NULL engine");
  if (!coef_host) {
    e->sol_on = e->sol_noise = false;
    e->sol_n = 0;
    e->sol_coef.clear();
    e->sol_ctl.clear();
    e->sol_ids.clear();
    return 0;
  }
  FLUXMI_REQUIRE(!e->is_cn, "engine_set_solver: a ControlNet engine steps nothing (set the solver on the main engine)");
  FLUXMI_REQUIRE(e->ws, "engine_set_solver: call fluxmi_engine_prepare first (the program belongs to the prepared shape)");
  FLUXMI_REQUIRE(ctl_host, "engine_set_solver: coef_host and ctl_host go together");
  FLUXMI_REQUIRE(n >= 0 && n <= MAX_STEPS, "engine_set_solver: n=%d out of range (at most %d evaluations)", n, MAX_STEPS);
  for (int i = 0; i < 8 * n; ++i)  // (checked as the device sees it: a finite double above FLT_MAX is inf in the fp32 table)
    FLUXMI_REQUIRE(std::isfinite((float)coef_host[i]), "engine_set_solver: coefficient %d of row %d is not finite in fp32", i % 8, i / 8);
  for (int i = 0; i < 4 * n; ++i)
    FLUXMI_REQUIRE(i % 4 == 0 || (ctl_host[i] >= -1 && ctl_host[i] <= 1), "engine_set_solver: slot %d of row %d is %d (a slot is -1, 0 or 1)",
                   i % 4, i / 4, ctl_host[i]);
  e->sol_coef.resize((size_t)8 * n);
  for (int i = 0; i < 8 * n; ++i) e->sol_coef[i] = (float)coef_host[i];
  e->sol_ctl.assign(ctl_host, ctl_host + 4 * n);
  e->sol_n = n;
  e->sol_on = true;
  e->sol_noise = false;  // a new program: its noise, if it has any, is set after it
  e->sol_ids.clear();
  return 0;
}

// The noise ids and evaluation offset of the program just set (fluxmi.h): host data only, like the program itself.
int fluxmi_engine_set_solver_noise(fluxmi_engine_t* e, const unsigned* ids_host, int batch, int eval_offset) {
  FLUXMI_REQUIRE(e && ids_host, "engine_set_solver_noise: NULL argument");
  FLUXMI_REQUIRE(e->ws && e->sol_on, "engine_set_solver_noise: call fluxmi_engine_set_solver first (the noise belongs to its program)");
  bool cn = false;
  for (int i = 0; i < e->sol_n; ++i) cn = cn || e->sol_coef[(size_t)8 * i + 7] != 0.f;
  FLUXMI_REQUIRE(cn, "engine_set_solver_noise: the solver program has no non-zero noise coefficient (column 7): it draws nothing");
  FLUXMI_REQUIRE(batch >= 1 && batch <= e->B, "engine_set_solver_noise: batch %d outside 1..%d (the prepared batch)", batch, e->B);
  FLUXMI_REQUIRE(eval_offset >= 0, "engine_set_solver_noise: eval_offset %d < 0", eval_offset);
  e->sol_ids.assign(ids_host, ids_host + 4 * (size_t)batch);
  e->sol_noise_B = batch;
  e->sol_eval_offset = eval_offset;
  e->sol_noise = true;
  return 0;
}

// The guidance-shaping state of the following guided denoise calls (fluxmi.h): host data only, like the solver program.
int fluxmi_engine_set_guidance(fluxmi_engine_t* e, const float* params_host, int step_offset) {
  FLUXMI_REQUIRE(e, "engine_set_guidance: NULL engine");
  if (!params_host) {
    e->gd_on = e->gd_zero_r = false;
    return 0;
  }
  FLUXMI_REQUIRE(!e->is_cn, "engine_set_guidance: a ControlNet engine steps nothing (set the shaping on the main engine)");
  FLUXMI_REQUIRE(e->ws, "engine_set_guidance: call fluxmi_engine_prepare first (the state belongs to the prepared shape)");
  for (int i = 0; i < 8; ++i) FLUXMI_REQUIRE(std::isfinite(params_host[i]), "engine_set_guidance: parameter %d is not finite", i);
  const float phi = params_host[1], rho = params_host[3], mode = params_host[5], zi = params_host[6];
  FLUXMI_REQUIRE(mode == 0.f || mode == 1.f || mode == 2.f, "engine_set_guidance: mode %g (0 = CFG, 1 = APG, 2 = CFG-Zero*)", (double)mode);
  FLUXMI_REQUIRE(phi >= 0.f && phi <= 1.f, "engine_set_guidance: phi %g outside [0, 1] (the rescale blend)", (double)phi);
  FLUXMI_REQUIRE(rho >= 0.f && zi >= 0.f, "engine_set_guidance: rho %g, zero_init %g must be >= 0 (0 = off)", (double)rho, (double)zi);
  FLUXMI_REQUIRE(step_offset >= 0, "engine_set_guidance: step_offset %d < 0", step_offset);
  memcpy(e->gd_params, params_host, 32);
  e->gd_params[7] = 0.f;
  e->gd_offset = step_offset;
  e->gd_on = e->gd_zero_r = true;
  return 0;
}

// The progress / preview / cancellation state of the following denoise calls (fluxmi.h): host data only, like the solver program; the pinned
// delivery buffer, the private copy stream and the event ring are made here, never inside a denoise call.
int fluxmi_engine_set_preview(fluxmi_engine_t* e, const float* proj51_host, int h, int w, int every, int eval_offset, int n_evaluations,
                              fluxmi_step_hook_t hook, void* user) {
  FLUXMI_REQUIRE(e, "engine_set_preview: NULL engine");
  if (!hook) {
    e->pv_hook = nullptr; e->pv_user = nullptr; e->pv_every = 0;
    return 0;
  }
  FLUXMI_REQUIRE(!e->is_cn, "engine_set_preview: a ControlNet engine steps nothing (set the hook on the main engine)");
  FLUXMI_REQUIRE(e->ws, "engine_set_preview: call fluxmi_engine_prepare first (the state belongs to the prepared shape)");
  FLUXMI_REQUIRE(!e->amax_hook, "engine_set_preview: an amax-exchange hook is attached (previews, progress and cancellation are refused under a "
                 "process group: the host waits would stall its collectives)");
  FLUXMI_REQUIRE(every >= 0, "engine_set_preview: every %d < 0 (0 = progress and cancellation only)", every);
  FLUXMI_REQUIRE(eval_offset >= 0 && n_evaluations >= 0, "engine_set_preview: eval_offset %d, n_evaluations %d must be >= 0", eval_offset, n_evaluations);
  if (every > 0) {
    FLUXMI_REQUIRE(proj51_host, "engine_set_preview: every > 0 needs the 51 projection floats");
    for (int i = 0; i < 51; ++i) FLUXMI_REQUIRE(std::isfinite(proj51_host[i]), "engine_set_preview: projection value %d is not finite", i);
    FLUXMI_REQUIRE(c_out(e) == 64, "engine_set_preview: the model predicts %d channels per token (a preview needs 16 latent channels x 4 sub-pixels)", c_out(e));
    FLUXMI_REQUIRE(h >= 1 && w >= 1 && (long long)h * w == e->Lpred, "engine_set_preview: a token grid of %d x %d for the %d stepped rows of the "
                   "prepared shape", h, w, e->Lpred);
    const size_t need = (size_t)e->B * e->Lpred * 4 * 3;
    if (e->pv_host_bytes < need) {
      if (e->pv_host) { hipHostFree(e->pv_host); e->pv_host = nullptr; e->pv_host_bytes = 0; }
      FLUXMI_CHECK_HIP(hipHostMalloc((void**)&e->pv_host, need, hipHostMallocDefault));
      e->pv_host_bytes = need;
    }
    if (!e->pv_stream) FLUXMI_CHECK_HIP(hipStreamCreateWithFlags(&e->pv_stream, hipStreamNonBlocking));
    memcpy(e->pv_proj, proj51_host, 51 * 4);
  }
  for (hipEvent_t& ev : e->pv_ev)
    if (!ev) FLUXMI_CHECK_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  e->pv_h = every > 0 ? h : 0;
  e->pv_w = every > 0 ? w : 0;
  e->pv_every = every;
  e->pv_offset = eval_offset;
  e->pv_n = n_evaluations;
  e->pv_hook = hook;
  e->pv_user = user;
  return 0;
}

int fluxmi_engine_preview_stats(fluxmi_engine_t* e, long long* captures, int* evaluations_run) {
  FLUXMI_REQUIRE(e && captures && evaluations_run, "engine_preview_stats: NULL argument");
  *captures = e->captures;
  *evaluations_run = e->pv_launched;
  return 0;
}

// The IP-Adapter of the prepared shape (fluxmi.h): K / V are copied into the engine's own buffer on `stream`, in order with the forward /
// denoise call that follows on it; the scales are staged behind them.
int fluxmi_engine_set_ip_adapter(fluxmi_engine_t* e, const void* k_ip, const void* v_ip, int Nk, int batch, const float* scales_host, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  FLUXMI_REQUIRE(e, "engine_set_ip_adapter: NULL engine");
  if (!k_ip) {
    e->ip_on = false;
    return 0;
  }
  FLUXMI_REQUIRE(!e->is_cn, "engine_set_ip_adapter: a ControlNet engine takes no IP-Adapter (set it on the main engine)");
  FLUXMI_REQUIRE(e->ws, "engine_set_ip_adapter: call fluxmi_engine_prepare first (the adapter belongs to the prepared shape)");
  FLUXMI_REQUIRE(v_ip && scales_host, "engine_set_ip_adapter: NULL v_ip / scales_host");
  FLUXMI_REQUIRE(Nk >= 1 && Nk <= 64, "engine_set_ip_adapter: Nk = %d outside 1..64", Nk);
  FLUXMI_REQUIRE(batch == e->B, "engine_set_ip_adapter: K / V for %d samples on a prepared batch of %d (a guided request carries both branches)",
                 batch, e->B);
  FLUXMI_REQUIRE(e->d.depth >= 1 && e->d.hidden == e->d.heads * 128, "engine_set_ip_adapter: the adapter needs double blocks and head_dim 128");
  FLUXMI_REQUIRE(!e->masked, "engine_set_ip_adapter: a token-group attention table is set (regional prompts do not combine with an IP-Adapter)");
  FLUXMI_REQUIRE(!(e->fb_threshold > 0.f), "engine_set_ip_adapter: step caching is on (it does not combine with an IP-Adapter)");
  const size_t kv = (size_t)e->d.depth * batch * Nk * e->d.hidden * 2, sc = (size_t)batch * e->d.depth * 4, total = 2 * kv + sc;
  SideBuf& mem = e->side[SB_IP];
  if (!mem.p || mem.bytes < total) {
    e->ip_on = false;
    if (mem.p) {  // a captured graph may hold the old buffer: never free it under a replay in flight
      FLUXMI_CHECK_HIP(hipDeviceSynchronize());
      mem.drop(e);
    }
    FLUXMI_TRY(mem.alloc(total, false, s, "engine_set_ip_adapter", ""));
    e->ip_gen = next_generation();
  }
  // the layout follows Nk (k | v | scales packed for THIS Nk): Nk is part of the graph key
  FLUXMI_CHECK_HIP(hipMemcpyAsync(mem.p, k_ip, kv, hipMemcpyDeviceToDevice, s));
  FLUXMI_CHECK_HIP(hipMemcpyAsync(mem.p + kv, v_ip, kv, hipMemcpyDeviceToDevice, s));
  FLUXMI_CHECK_HIP(hipStreamSynchronize(s));  // (the previous staging copy, if any, has left ip_scales_h)
  e->ip_scales_h.assign(scales_host, scales_host + (size_t)batch * e->d.depth);
  FLUXMI_CHECK_HIP(hipMemcpyAsync(mem.p + 2 * kv, e->ip_scales_h.data(), sc, hipMemcpyHostToDevice, s));
  e->ip_nk = Nk;
  e->ip_B = batch;
  e->ip_on = true;
  return 0;
}

int fluxmi_engine_set_step_cache(fluxmi_engine_t* e, float threshold, int max_consecutive_hits) {
  FLUXMI_REQUIRE(e, "engine_set_step_cache: NULL engine");
  FLUXMI_REQUIRE(threshold >= 0.f, "engine_set_step_cache: threshold %g must be >= 0 and not NaN (0 = off)", (double)threshold);
  FLUXMI_REQUIRE(max_consecutive_hits >= 0, "engine_set_step_cache: max_consecutive_hits %d must be >= 0 (0 = unbounded)", max_consecutive_hits);
  e->fb_threshold = threshold;
  e->fb_max_hits = max_consecutive_hits;
  return 0;
}

int fluxmi_engine_step_cache_log(fluxmi_engine_t* e, int* n, int* batch, float* ratios, unsigned char* hit, int cap) {
  FLUXMI_REQUIRE(e && n && batch && cap >= 0 && (cap == 0 || (ratios && hit)), "engine_step_cache_log: bad arguments");
  const int steps = (int)e->fb_log_hit.size(), m = std::min(steps, cap);
  *n = steps;
  *batch = steps ? e->fb_log_B : 0;
  for (int i = 0; i < m; ++i) hit[i] = e->fb_log_hit[i];
  for (long long i = 0; i < (long long)m * e->fb_log_B; ++i) ratios[i] = e->fb_log_ratio[i];
  return 0;
}

}  // extern "C"
