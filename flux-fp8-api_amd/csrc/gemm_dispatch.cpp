// fluxmi -- GEMM dispatch: which launches a grouped GEMM becomes.  Host-only translation unit.
//
// Three layers: the predicates over the tile-config table (gemm_cfg.h), the PLANNER -- a pure function from (groups, shape, operand format,
// epilogue, one tuning snapshot, batch, split-K block) to a list of launches, no HIP call, no global read -- and the EXECUTOR, which walks that
// list and calls the launchers.  fluxmi_gemm_dispatch = planner + executor; fluxmi_gemm_plan (include/fluxmi.h) exports the planner, so a
// dispatch decision can be read and tested without a GPU (tests/test_gemm_plan_cpu.py).
#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "fluxmi_internal.h"
#include "gemm_cfg.h"

int fluxmi_gemm_tile_ok(int N, int K, int is_fp8, int cfg) {
  const GemmTileCfg* c = gemm_cfg(cfg);
  const int kb = K * (is_fp8 ? 1 : 2);
  return c && (N % c->bn == 0) && (kb % c->kstep == 0) && kb >= c->min_k;
}

// Whether tile config `cfg` runs launch `p` as it stands: the conditions fluxmi_launch_gemm and the per-config launchers REQUIRE (tiling, the
// split column, fused K / V^T outputs, the operand format and epilogue a config is compiled for, the persistent kernel's conditions).
// A forced tile config (fluxmi_tuning_t.gemm_cfg) is taken only where this holds; every other launch keeps the automatic choice.
static int fluxmi_gemm_cfg_supports(const FluxmiGemmParams& p, int is_fp8, int act_fmt, int cfg) {
  if (!fluxmi_gemm_tile_ok(p.N, p.K, is_fp8, cfg)) return 0;
  const GemmTileCfg& c = *gemm_cfg(cfg);
  if (p.epi == FLUXMI_EPI_SPLIT && p.g[0].split_n % c.bn != 0) return 0;
  bool fused_out = false;
  for (int i = 0; i < p.n_groups; ++i) fused_out |= (p.g[i].vt_out != nullptr || p.g[i].k_out != nullptr);
  if (fused_out && !c.fused_kv) return 0;
  if (c.family == GEMM_FAMILY_PERSISTENT) return fluxmi_gemm_persist_ok(p, is_fp8, act_fmt);
  return gemm_cfg_takes(c, is_fp8, act_fmt, p.epi);
}

// mods_gemm (engine.hip) needs results that do not depend on how many rows share a launch (the step-ahead table of R = steps x B rows
// must equal the per-step R = B launches bit for bit): it switches the M-dependent split-K choice off around its launches
static thread_local int g_splitk_block = 0;
void fluxmi_gemm_block_splitk(int on) { g_splitk_block += on ? 1 : -1; }

// The split-K choice of a bf16 launch depends on how many tiles the launch has, and a split-K sum associates K differently from the
// one-pass kernels (whose tile configs all give the same bits): decided on ALL rows of a batched launch, a sample's result would follow the
// batch it rides in (Flux-schnell 256^2, bf16 flow: split-K at B = 1, none from B = 4 on).  An engine therefore announces its batch
// (fluxmi_gemm_set_batch, thread-local like the scratch pointers) and the planner decides on ONE sample's share of the groups;
// reference flux_model.py:672-716 has no cross-sample operation.
static thread_local int g_gemm_batch = 1;
void fluxmi_gemm_set_batch(int B) { g_gemm_batch = B < 1 ? 1 : B; }

namespace {

enum { LAUNCH_TILE = 0, LAUNCH_GENERIC = 1, LAUNCH_SPLITK = 2 };  // the `kind` of fluxmi_gemm_plan's encoding
struct Launch {
  int kind, cfg, S;         // tile config (LAUNCH_TILE) / split-K slices (LAUNCH_SPLITK), else -1 / 0
  std::vector<int> groups;  // indices into the caller's groups, in launch order; at most FLUXMI_MAX_GROUPS
};

constexpr size_t SPLITK_CAP = FLUXMI_SPLITK_WS_BYTES;
FluxmiGemmParams params_of(const FluxmiGemmGroup* gs, const int* ix, int n, int N, int K, int epi) {  // the launch descriptor of groups ix[0 .. n)
  FluxmiGemmParams p;
  memset(&p, 0, sizeof(p));
  for (int i = 0; i < n; ++i) p.g[i] = gs[ix[i]];
  p.n_groups = n; p.N = N; p.K = K; p.epi = epi;
  return p;
}
long long tiles_m(int M, int bm) { return (M + bm - 1) / bm; }

struct Planner {
  const FluxmiGemmGroup* gs;
  int N, K, is_fp8, act_fmt, epi;
  fluxmi_tuning_t tun;  // ONE snapshot, taken by the caller
  int batch;
  bool splitk_block;
  std::vector<Launch> out;

  long long tiles_of(const int* ix, int n, int bm, int bn) const {  // tiles of a bm x bn tiling of groups ix[0 .. n)
    long long t = 0;
    for (int i = 0; i < n; ++i) t += tiles_m(gs[ix[i]].M, bm);
    return t * (N / bn);
  }
  bool tile_ok(int cfg) const { return fluxmi_gemm_tile_ok(N, K, is_fp8, cfg) != 0; }
  bool plain_epi() const { return epi == FLUXMI_EPI_BF16 || epi == FLUXMI_EPI_GATE_RESID; }
  void emit(int kind, int cfg, int S, const int* ix, int n) { out.push_back({kind, cfg, S, std::vector<int>(ix, ix + n)}); }

  // Tile choice: minimise (#waves of tiles over the 256 CUs) x (per-tile cost).  Relative per-tile efficiencies were measured on MI355X
  // (profiles/r01_kernel_sweep.txt); fluxmi_tuning_t.gemm_cfg overrides.
  int auto_cfg(const FluxmiGemmParams& p, const int* ix) const {
    // a forced tile config (FLUXMI_GEMM_CFG) is taken where it applies: where the launch's shape, outputs, operand format and epilogue are
    // ones that config runs (fluxmi_gemm_cfg_supports); any other launch falls back to the cost model below instead of failing in the
    // launcher.  The persistent kernel is applied by chunk(), after the splitting decisions
    const int forced = tun.gemm_cfg;
    if (forced >= 0 && !gemm_cfg_is(forced, GEMM_FAMILY_PERSISTENT) && fluxmi_gemm_cfg_supports(p, is_fp8, act_fmt, forced)) return forced;
    // candidates, in order of preference at equal cost; eff = measured relative rate per flop on MI355X at full occupancy
    // (profiles/r01_kernel_sweep.txt).  Cost = (number of block waves) x (time of one wave of blocks).
    // The one-wave-per-SIMD kernel (128x128 wave tiles): the leaner main loop wins once K is long enough to amortise its
    // twice-as-long per-wave epilogue (measured +6 % at K = 15360, -5 % at K = 3072)
    const bool long_k = (long long)K * (is_fp8 ? 1 : 2) >= 8192;
    constexpr int NC = 4;
    static const int cand[NC] = {GEMM_CFG_PP, GEMM_CFG_W1, GEMM_CFG_T128, GEMM_CFG_T128x64};
    const double eff[NC] = {1.00, long_k ? 1.06 : 0.94, 0.84, 0.30};
    int best = -1;
    double best_cost = 1e300;
    for (int ci = 0; ci < NC; ++ci) {
      if (!tile_ok(cand[ci])) continue;
      const GemmTileCfg& c = *gemm_cfg(cand[ci]);
      const long long tiles = tiles_of(ix, p.n_groups, c.bm, c.bn);
      const long long slots = 256LL * c.wgs_per_cu;
      const long long waves = (tiles + slots - 1) / slots;
      // a last wave that fills less than half of a 2-blocks/CU machine runs its blocks alone on their CUs (~1.6x faster)
      double w = (double)waves;
      if (c.wgs_per_cu == 2 && tiles - (waves - 1) * slots <= 256) w -= 0.4;
      const double cost = w * c.wgs_per_cu * (double)c.bm * c.bn / eff[ci];
      if (cost < best_cost) { best_cost = cost; best = c.id; }
    }
    return best;
  }

  // split-K slices for a bf16 launch (0 = one pass); `tiles`, `rows`: 256-row tiles x N / 256 and padded rows of its groups
  int splitk_slices(long long tiles, long long rows, bool fused_out, int force_cfg) const {
    const int nk = K * (is_fp8 ? 1 : 2) / 64;
    const bool can = !fused_out && plain_epi() && tile_ok(GEMM_CFG_PP) && tiles > 0;
    int S = 0;
    // measured on M = 512 bf16 launches (tools/bf16_gemm_probe.py, profiles/r03_small_m.txt): below ~190 K-steps per tile the 128x128 tiles at two
    // workgroups per CU are as fast as any split; above, ~40-50 K-steps per workgroup is the sweet spot (K = 15360: 72 us vs 158 us unsplit)
    if (force_cfg < 0 && tun.gemm_splitk && !splitk_block && can && !is_fp8 && tun.gemm_cfg < 0 && tiles <= 128 && nk >= 192)
      S = (int)std::max<long long>(2, std::min<long long>(std::min<long long>(256 / tiles, (nk + 24) / 48), 16));
    while (S >= 2 && (size_t)S * rows * N * 4 > SPLITK_CAP) --S;
    return S >= 2 ? S : 0;
  }

  // One launch's worth of groups (n <= FLUXMI_MAX_GROUPS).  force_cfg >= 0: the caller's tile config where it tiles the shape.
  // s_hint: -1 = decide the split-K slices on this chunk's own groups; >= 0 = decided by the caller on one sample's groups (0: one pass)
  int chunk(const int* ix, int n, int force_cfg, int s_hint) {
    const FluxmiGemmParams p = params_of(gs, ix, n, N, K, epi);
    int cfg = force_cfg >= 0 && tile_ok(force_cfg) ? force_cfg : auto_cfg(p, ix);
    const bool auto_tiles = force_cfg < 0 && tun.gemm_cfg < 0;  // neither the caller nor the knob names a config
    if (force_cfg < 0 && gemm_cfg_is(tun.gemm_cfg, GEMM_FAMILY_PERSISTENT) && tile_ok(GEMM_CFG_PP) && fluxmi_gemm_persist_ok(p, is_fp8, act_fmt))
      cfg = tun.gemm_cfg;
    bool fused_out = false;
    long long rows = 0;
    for (int i = 0; i < n; ++i) { rows += tiles_m(p.g[i].M, 256) * 256; fused_out |= (p.g[i].vt_out || p.g[i].k_out); }
    const long long t256 = tiles_of(ix, n, 256, 256);
    // small-M launches (M <= 512: schnell 256x256, the text encoders, the modulation GEMMs): 24-96 tiles of 256x256 for 256 CUs, weight-stream
    // bound -> split K over several workgroups per tile (fp32 partials + a reduce / epilogue pass).  fluxmi_tuning_t.gemm_splitk = 0 turns it off;
    // fluxmi_gemm_grouped(tile_cfg = 113 + S) forces S splits (tests).
    const int S = s_hint >= 0 ? s_hint : splitk_slices(t256, rows, fused_out, force_cfg);
    if (S >= 2) {
      // the fp32 partial tiles of S slices must fit the scratch: a batched launch whose S was fixed on one sample goes in as many pieces as it takes
      if ((size_t)S * rows * N * 4 <= SPLITK_CAP) { emit(LAUNCH_SPLITK, -1, S, ix, n); return 0; }
      FLUXMI_REQUIRE(s_hint >= 0, "gemm: split-K scratch too small for %d slices", S);
      for (int i0 = 0; i0 < n;) {
        const int first = i0;
        size_t r = 0;
        while (i0 < n) {
          const size_t gr = (size_t)tiles_m(p.g[i0].M, 256) * 256;
          if (i0 > first && (size_t)S * (r + gr) * N * 4 > SPLITK_CAP) break;
          FLUXMI_REQUIRE((size_t)S * gr * N * 4 <= SPLITK_CAP, "gemm: one group of %d rows does not fit the split-K scratch at %d slices", p.g[i0].M, S);
          ++i0;
          r += gr;
        }
        emit(LAUNCH_SPLITK, -1, S, ix + first, i0 - first);
      }
      return 0;
    }
    // bf16 operands, one thin round of 256x256 tiles (Flux-schnell linear1 at M = 512: 168 tiles): the one-wave-per-SIMD kernel runs the
    // single tile per CU fastest (74 us vs 95 / 98 us for the ping-pong / 128x128 kernels, profiles/r03_small_m.txt)
    if (!is_fp8 && auto_tiles && tile_ok(GEMM_CFG_W1)) {
      if (t256 > 128 && t256 <= 256 && (!fused_out || cfg == GEMM_CFG_PP)) cfg = GEMM_CFG_W1;
      // ... and on 192-row tiles when those still fit one round (M = 512, N = 21504: 3 x 84 = 252 tiles of three quarters the work instead of 168)
      if (cfg == GEMM_CFG_W1 && !fused_out && plain_epi() && tun.gemm_tile192) {
        const long long t192 = tiles_of(ix, n, 192, 256);
        if (t192 <= 256 && t192 > t256) cfg = GEMM_CFG_W1_192;
      }
    }
    // multi-round fp8 launches of the step (single-block linear1: 5.9 rounds of the 256 CUs, double-block mlp.0: 3.0, qkv: 2.25): one
    // persistent workgroup per CU walks the tiles -- no workgroup relaunch, cold prologue or store drain per tile (gemm_persist.hip).
    // Single-round launches gain nothing from it and keep the one-tile-per-workgroup kernel.
    if (cfg == GEMM_CFG_PP && tun.gemm_persist && tun.gemm_cfg < 0 && fluxmi_gemm_persist_ok(p, is_fp8, act_fmt) && t256 > 256)
      cfg = tun.gemm_persist == 2 ? GEMM_CFG_PERSIST_TIMING : GEMM_CFG_PERSIST;  // 2: the timing build (probes: fluxmi_gemm_debug_buffer)
    // gate*y+x launches of the one-wave-per-SIMD kernel whose 256-row tiling fills less than one round of the 256 CUs: lower tiles of the same
    // kernel (same bits).  Flux-dev 768^2 (M = 2816 -> 11 x 12 = 132 tiles on mlp.2 / linear2): 192-row tiles are three quarters of
    // the work each and 15 x 12 = 180 of them still run in one round (round 5, -13.6 % per launch).  Flux-dev 1024^2 linear2 (M = 4608 -> 216
    // tiles): 224-row tiles (round 6: the four waves side by side along N) give 21 x 12 = 252 tiles = one round at 7/8 of the work
    // (isolated, cold operands: 203.7 -> 181.0 us).  Cost = rounds x tile height x a per-height factor for the fragment bytes per MFMA (the
    // 192-row 2 x 2 grid reads 8 % more, the 224-row 1 x 4 grid 29 % more but keeps all four SIMDs equally loaded); taken when it drops by more
    // than 5 %.  fluxmi_tuning_t.gemm_tile192 = 0 turns both off, 2 = 192-row tiles only (A/B of the round-6 heights).
    const bool f8_gate = is_fp8 && act_fmt == FLUXMI_E5M2 && epi == FLUXMI_EPI_GATE_RESID;
    if (cfg == GEMM_CFG_W1 && auto_tiles && f8_gate && tun.gemm_tile192) {
      const bool round6 = tun.gemm_tile192 == 1;
      const struct { int cfg; double work, frag; bool on; } lower[] = {{GEMM_CFG_W1_192, 0.75, 1.04, true},
                                                                       {GEMM_CFG_W1_224, 0.875, 1.03, round6},
                                                                       {GEMM_CFG_W1_160, 0.625, 1.08, round6}};  // 768^2: 18 x 12 = 216 tiles
      double best = 0.95 * (double)((t256 + 255) / 256);
      for (const auto& l : lower) {
        if (!l.on || !tile_ok(l.cfg)) continue;
        const double c = (double)((tiles_of(ix, n, gemm_cfg(l.cfg)->bm, 256) + 255) / 256) * l.work * l.frag;
        if (c < best) { best = c; cfg = l.cfg; }
      }
    }
    const bool split_ok = epi != FLUXMI_EPI_SPLIT || cfg < 0 || (p.g[0].split_n % gemm_cfg(cfg)->bn == 0);
    if (cfg < 0 || !split_ok) emit(LAUNCH_GENERIC, -1, 0, ix, n);
    else emit(LAUNCH_TILE, cfg, 0, ix, n);
    return 0;
  }

  int chunks(const std::vector<int>& v, int force_cfg, int s_hint) {
    for (size_t off = 0; off < v.size(); off += FLUXMI_MAX_GROUPS)
      FLUXMI_TRY(chunk(v.data() + off, (int)std::min<size_t>(FLUXMI_MAX_GROUPS, v.size() - off), force_cfg, s_hint));
    return 0;
  }

  // How many of the smallest groups (row counts `ms`, ascending) are peeled into a 128x128 launch at two workgroups per CU, because the 256x256
  // tiling leaves a thin last round of tiles (e.g. double-block mlp.0 at 768^2).  Results do not depend on the tile shape.
  int peel_count(const std::vector<int>& ms, bool peel_ok) const {
    if (!peel_ok || ms.size() < 2 || ms.size() > FLUXMI_MAX_GROUPS) return 0;
    const long long tn = N / 256;
    long long T = 0;
    for (int m : ms) T += tiles_m(m, 256) * tn;
    // multi-round fp8 launches run on the PERSISTENT kernel, whose last, partial round costs what its tiles cost: peeling only pays when that
    // round is thin.  Measured in-step after the row-pair activations (profiles/r06_act_pairs.txt section 5): Flux-dev 1024^2 mlp.0, 864 tiles
    // = 3 rounds + 96 tiles (37 % of a round): the peel LOSES 0.4 % per step; 768^2, 528 tiles = 2 rounds + 16 tiles: it gains 1.9 %
    if (is_fp8 && act_fmt == FLUXMI_E5M2 && tun.gemm_persist && T > 256 && T % 256 > 64) return 0;
    double best = (double)((T + 255) / 256) - 0.15;
    int best_k = 0;
    long long peeled = 0;
    for (size_t k = 1; k < ms.size(); ++k) {  // peel the k smallest groups
      peeled += tiles_m(ms[k - 1], 256) * tn;
      long long small_tiles = 0;
      for (size_t q = 0; q < k; ++q) small_tiles += tiles_m(ms[q], 128) * (N / 128);
      const double cost = (double)((T - peeled + 255) / 256) + 0.58 * (double)((small_tiles + 511) / 512);
      if (cost < best) { best = cost; best_k = (int)k; }
    }
    return best_k;
  }

  int plan(int n_in) {
    std::vector<int> all(n_in);
    for (int i = 0; i < n_in; ++i) all[i] = i;
    bool fused_attn = false;
    for (int i : all) fused_attn |= (gs[i].vt_out != nullptr || gs[i].k_out != nullptr);
    if (fused_attn) {
      // the attention-layout epilogue lives in the LDS-transposed epilogue of the 256x256 kernels only
      const bool long_k = (long long)K * (is_fp8 ? 1 : 2) >= 8192;
      const int cfg = (long_k && tile_ok(GEMM_CFG_W1)) ? GEMM_CFG_W1 : GEMM_CFG_PP;
      FLUXMI_REQUIRE(tile_ok(cfg), "gemm: fused K / V^T outputs need N %% 256 == 0 and K*bytes %% 64 == 0 (N=%d K=%d)", N, K);
      for (int i : all) {
        const FluxmiGemmGroup& g = gs[i];
        FLUXMI_REQUIRE(g.heads > 0 && g.kv_col0 % 128 == 0 && g.tok0 % 16 == 0 && g.vt_rows % 8 == 0 && g.vt_ld % 8 == 0 &&
                           (!g.k_out || (g.kv_col0 % 256 == 0 && (g.heads * 128) % 256 == 0 && g.pe && g.k_norm && g.k_rows > 0)),
                       "gemm: fused K / V^T outputs need tok0 %% 16 == 0, vt_rows %% 8 == 0, vt_ld %% 8 == 0 (K: 256-aligned q|k|v blocks, pe, k_norm)");
      }
      return chunks(all, cfg, -1);
    }
    const bool peel_ok = tun.gemm_hybrid && tun.gemm_cfg < 0 && tile_ok(GEMM_CFG_PP) && tile_ok(GEMM_CFG_T128) &&
                         (epi != FLUXMI_EPI_SPLIT || gs[0].split_n % 256 == 0);
    // bf16 launches of a batched engine (fluxmi_gemm_set_batch): replay the decisions of ONE sample's launch -- which groups are peeled, how many
    // split-K slices the others get -- and apply them to every sample's groups.  One sample's share = 1 / batch of the groups of every row
    // count (the engine pushes one group per (sample, stream)), or 1 / batch of the rows of a single group that carries the whole batch.  The
    // one-pass tile configs all give the same bits, so only the split-K slices have to follow the sample; a launch whose groups do not divide
    // by the batch keeps the whole-launch decision.
    if (!is_fp8 && batch > 1) {
      const int B = batch;
      bool ok = true;
      std::vector<int> rows_all, sub;  // row counts of the launch / of one sample's share, ascending
      std::map<int, int> per_sample;   // rows of a group of the launch -> rows of it that belong to one sample
      for (int i : all) rows_all.push_back(gs[i].M);
      std::sort(rows_all.begin(), rows_all.end());
      for (size_t i = 0; i < rows_all.size() && ok;) {
        size_t j = i;
        while (j < rows_all.size() && rows_all[j] == rows_all[i]) ++j;
        const size_t cnt = j - i;
        if (cnt % B == 0) { sub.insert(sub.end(), cnt / B, rows_all[i]); per_sample[rows_all[i]] = rows_all[i]; }
        else if (cnt == 1 && rows_all[i] % B == 0) { sub.push_back(rows_all[i] / B); per_sample[rows_all[i]] = rows_all[i] / B; }
        else ok = false;
        i = j;
      }
      std::sort(sub.begin(), sub.end());
      const int k = ok ? peel_count(sub, peel_ok) : 0;
      if (ok && k > 0 && k < (int)sub.size() && sub[k - 1] == sub[k]) ok = false;  // the peel would cut through groups of one row count
      // one sample's launch decides per chunk of FLUXMI_MAX_GROUPS groups; a sample has a handful, so its launch is one chunk
      if (ok && sub.size() <= FLUXMI_MAX_GROUPS) {
        const int m_small = k > 0 ? sub[k - 1] : -1;  // groups of at most this many rows (per sample) are peeled
        long long tiles = 0, rows = 0;
        for (size_t q = (size_t)k; q < sub.size(); ++q) { tiles += tiles_m(sub[q], 256); rows += tiles_m(sub[q], 256) * 256; }
        const int S = splitk_slices(tiles * (N / 256), rows, false, -1);
        std::vector<int> big, small;
        for (int i : all) (per_sample[gs[i].M] <= m_small ? small : big).push_back(i);
        FLUXMI_TRY(chunks(big, -1, S));
        return chunks(small, GEMM_CFG_T128, 0);
      }
    }
    if (peel_ok && all.size() >= 2 && all.size() <= FLUXMI_MAX_GROUPS) {
      std::vector<int> order = all;
      std::sort(order.begin(), order.end(), [&](int a, int b) { return gs[a].M < gs[b].M; });
      std::vector<int> ms;
      for (int i : order) ms.push_back(gs[i].M);
      const int best_k = peel_count(ms, peel_ok);
      if (best_k > 0) {
        // (running the thin launch on a side stream BESIDE the big one, fork / join through events, was measured slower: 45.47 vs
        // 45.13 ms per step, profiles/r02_gemm_ab.txt -- its workgroups take CUs from the big grid's first rounds, not its last)
        FLUXMI_TRY(chunk(order.data() + best_k, (int)order.size() - best_k, -1, -1));
        return chunk(order.data(), best_k, GEMM_CFG_T128, -1);
      }
    }
    return chunks(all, -1, -1);
  }
};

int make_plan(const FluxmiGemmGroup* gs, int n, int N, int K, int is_fp8, int act_fmt, int epi, int batch, std::vector<Launch>& out) {
  Planner pl{gs, N, K, is_fp8, act_fmt, epi, fluxmi_tuning(), batch < 1 ? 1 : batch, g_splitk_block > 0, {}};
  FLUXMI_TRY(pl.plan(n));
  out.swap(pl.out);
  return 0;
}

}  // namespace

// One grouped GEMM of any number of groups: plan, then launch what the plan says.
int fluxmi_gemm_dispatch(const FluxmiGemmGroup* gs, int n, int N, int K, int is_fp8, int act_fmt, int epi, hipStream_t s) {
  std::vector<Launch> plan;
  FLUXMI_TRY(make_plan(gs, n, N, K, is_fp8, act_fmt, epi, g_gemm_batch, plan));
  for (const Launch& l : plan) {
    FluxmiGemmParams p = params_of(gs, l.groups.data(), (int)l.groups.size(), N, K, epi);
    FLUXMI_TRY(l.kind == LAUNCH_SPLITK    ? fluxmi_launch_gemm_splitk(p, is_fp8, act_fmt, l.S, s)
               : l.kind == LAUNCH_GENERIC ? fluxmi_launch_gemm_generic(p, is_fp8, act_fmt, s)
                                          : fluxmi_launch_gemm(p, is_fp8, act_fmt, l.cfg, s));
  }
  return 0;
}

int fluxmi_gemm_plan_export(const FluxmiGemmGroup* gs, int n, int N, int K, int is_fp8, int act_fmt, int epi, int batch, int* plan, int plan_cap,
                            int* plan_len) {
  FLUXMI_REQUIRE(gs && n >= 1 && N > 0 && K > 0 && plan_len && (plan || plan_cap == 0), "gemm_plan: bad arguments (n_groups=%d N=%d K=%d)", n, N, K);
  std::vector<Launch> launches;
  FLUXMI_TRY(make_plan(gs, n, N, K, is_fp8, act_fmt, epi, batch, launches));
  std::vector<int> flat;
  for (const Launch& l : launches) {
    flat.insert(flat.end(), {l.kind, l.cfg, l.S, (int)l.groups.size()});
    flat.insert(flat.end(), l.groups.begin(), l.groups.end());
  }
  *plan_len = (int)flat.size();
  FLUXMI_REQUIRE((int)flat.size() <= plan_cap, "gemm_plan: the plan needs %d integers, the caller has room for %d", (int)flat.size(), plan_cap);
  std::copy(flat.begin(), flat.end(), plan);
  return 0;
}
