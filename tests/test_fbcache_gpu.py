"""First-block step caching on the GPU (fluxmi.h, fluxmi_engine_set_step_cache).  On the rows the final layer reads,
with h0 / h1 the residual stream before / after double block 0:

    r = bf16(h1 - h0);  ratio_b = sum |r - r_ref| / sum |r_ref|  (fp32, fixed order, per sample);  r_ref = the r of the last full step
    hit  (a full step has run in this call, every ratio_b < threshold, fewer than cache_max_hits hits in a row):  x = bf16(h1 + R)
    miss: r_ref = r, the remaining blocks run, R = bf16(x_final - h1)

then the final layer and the update.  Tiny hidden-256 models and helpers are those of tests/test_cfg_gpu.py; the Python form of the loop is
tests/fbcache_util.py."""
import ctypes as C
import io
import math

import pytest
import torch

import fbcache_util as fu
import flux_oracle as fo
from test_cfg_gpu import (QUANTS, SCALE, build, cond_kw, inputs, make_oracle, prompts, rel_l2, tiny_config, tiny_pipeline, to_dev)

pytestmark = pytest.mark.gpu

CHUNK = 16384  # elements per workgroup of the metric pass (include/fluxmi.h)


def denoise(model, d, ts, img=None, guided=False, **kw):
    if guided:
        kw.update(neg_txt=d["neg_txt"], neg_y=d["neg_y"], cfg_scale=SCALE)
    return model.denoise(d["img"] if img is None else img, d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts, guidance=3.5, **cond_kw(d), **kw)


def ws_bytes(model):
    from fluxmi import _lib

    n = C.c_longlong(0)
    _lib.call("fluxmi_engine_workspace_bytes", model._engine, C.byref(n))
    return n.value


# ---- 1. the kernels against the torch expressions ---------------------------------------------------------------------------------------
def _metric(x, Lt, Lpred, h0, r_ref):
    """fluxmi_fb_metric on rows [Lt, Lt + Lpred) of x [B, L, H] -> (r, ratio, num, den)"""
    from fluxmi import _lib, ops

    B, L, H = x.shape
    n = Lpred * H
    r = torch.full_like(h0, 7.0)
    part = torch.zeros(B * ((n + CHUNK - 1) // CHUNK) * 2, dtype=torch.float32, device=x.device)
    ratio = torch.zeros(B, dtype=torch.float32, device=x.device)
    numden = torch.zeros(B, 2, dtype=torch.float32, device=x.device)
    _lib.call("fluxmi_fb_metric", ops._p(x[:, Lt:]), L * H, ops._p(h0), ops._p(r), ops._p(r_ref), ops._p(part), ops._p(ratio), ops._p(numden), B, n,
              ops._stream())
    torch.cuda.synchronize()
    return r, ratio, numden[:, 0], numden[:, 1]


@pytest.mark.parametrize("Lc", [0, 9], ids=["Lpred==Li", "Lpred<Li"])
@pytest.mark.parametrize("B", [1, 3])
def test_kernels_bit_exact_and_ratio_batch_invariant(dev, B, Lc):
    from fluxmi import _lib, ops

    H, Lt, Lpred = 256, 7, 150  # 150 rows x 256 = 2.34 workgroups' worth per sample: the last workgroup is ragged; odd Lt
    L = Lt + Lpred + Lc
    g = torch.Generator().manual_seed(3 + B + Lc)
    rnd = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).to(dev)
    x, h0, r_ref, h1, R = rnd(B, L, H), rnd(B, Lpred, H), rnd(B, Lpred, H), rnd(B, Lpred, H), rnd(B, Lpred, H)
    x0 = x.clone()
    rows, n, xs = x[:, Lt:Lt + Lpred], Lpred * H, L * H
    # snapshot
    snap = torch.zeros_like(h0)
    _lib.call("fluxmi_fb_snapshot", ops._p(x[:, Lt:]), xs, ops._p(snap), B, n, ops._stream())
    assert torch.equal(snap, rows)
    # metric: r bit for bit, num / den within 1e-5 of fp64 (a fixed-order fp32 tree over <= 2^24 non-negative terms errs by <= depth x 2^-24 ~ 1.5e-6)
    r, ratio, num, den = _metric(x, Lt, Lpred, h0, r_ref)
    want_r = rows - h0
    assert want_r.dtype == torch.bfloat16 and torch.equal(r, want_r)
    num64 = (want_r.double() - r_ref.double()).abs().sum(dim=(1, 2))
    den64 = r_ref.double().abs().sum(dim=(1, 2))
    for b in range(B):
        en, ed = abs(num[b].item() - num64[b].item()) / num64[b].item(), abs(den[b].item() - den64[b].item()) / den64[b].item()
        print(f"[fb_metric B={B} Lc={Lc} b={b}] num rel err {en:.2e} den rel err {ed:.2e} ratio {ratio[b].item():.6f}")
        assert en <= 1e-5 and ed <= 1e-5
        assert ratio[b].item() == (num[b] / den[b]).item()
    # in place over h0 (the engine's use), and launch after launch
    h0b = h0.clone()
    part = torch.zeros(B * ((n + CHUNK - 1) // CHUNK) * 2, dtype=torch.float32, device=dev)
    ratio2 = torch.zeros(B, dtype=torch.float32, device=dev)
    _lib.call("fluxmi_fb_metric", ops._p(x[:, Lt:]), xs, ops._p(h0b), ops._p(h0b), ops._p(r_ref), ops._p(part), ops._p(ratio2), None, B, n, ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(h0b, want_r) and torch.equal(ratio2, ratio)
    # a sample alone, as sample 0 and as sample 2 of a batch of 3: identical bits
    for b in range(B):
        one = _metric(x[b:b + 1].contiguous(), Lt, Lpred, h0[b:b + 1].contiguous(), r_ref[b:b + 1].contiguous())
        assert one[1][0].item() == ratio[b].item() and one[2][0].item() == num[b].item() and one[3][0].item() == den[b].item()
        for pos in (0, 2):
            x3, h3, f3 = rnd(3, L, H), rnd(3, Lpred, H), rnd(3, Lpred, H)
            x3[pos], h3[pos], f3[pos] = x[b], h0[b], r_ref[b]
            got = _metric(x3, Lt, Lpred, h3, f3)
            assert got[1][pos].item() == ratio[b].item() and got[2][pos].item() == num[b].item(), f"sample {b} at slot {pos} of 3"
    # den == 0 is a miss: +inf
    assert math.isinf(_metric(x, Lt, Lpred, h0, torch.zeros_like(r_ref))[1][0].item())
    # commit, store, apply
    rr, hh = torch.zeros_like(h0), torch.zeros_like(h0)
    _lib.call("fluxmi_fb_commit", ops._p(x[:, Lt:]), xs, ops._p(r), ops._p(rr), ops._p(hh), B, n, ops._stream())
    assert torch.equal(rr, r) and torch.equal(hh, rows)
    Rout = torch.zeros_like(h0)
    _lib.call("fluxmi_fb_store", ops._p(x[:, Lt:]), xs, ops._p(h1), ops._p(Rout), B, n, ops._stream())
    assert torch.equal(Rout, rows - h1)
    assert torch.equal(x, x0), "a read-only pass wrote x"
    want = h1 + R
    _lib.call("fluxmi_fb_apply", ops._p(x[:, Lt:]), xs, ops._p(h1), n, ops._p(R), B, n, ops._stream())
    assert torch.equal(x[:, Lt:Lt + Lpred], want)
    want2 = x[:, Lt:Lt + Lpred] + R
    _lib.call("fluxmi_fb_apply", ops._p(x[:, Lt:]), xs, ops._p(x[:, Lt:]), xs, ops._p(R), B, n, ops._stream())  # in place: h1 = x itself
    assert torch.equal(x[:, Lt:Lt + Lpred], want2)
    assert torch.equal(x[:, :Lt], x0[:, :Lt]) and torch.equal(x[:, Lt + Lpred:], x0[:, Lt + Lpred:]), "rows outside the cached range changed"
    with pytest.raises(RuntimeError, match="fb_store: bad shape"):
        _lib.call("fluxmi_fb_store", ops._p(x), xs, ops._p(h1), ops._p(Rout), B, n + 4, ops._stream())


# ---- the request of the model-level tests ------------------------------------------------------------------------------------------------
def frozen_request(dev, qname, kind, B=2, seed=5, steps=9, guided=False):
    """a tiny model calibrated by a 13-step request at the shape, then the frozen request: (model, d, ts2, start latents)"""
    cfg = tiny_config(kind)
    model, sd = build(cfg, QUANTS[qname], dev)
    d = to_dev(inputs(kind, cfg.params, 64, 64, 32, B, seed=seed), dev)
    ts = fo.get_schedule(16, d["img"].shape[1])
    lat = denoise(model, d, ts[:14], use_graph=False, guided=guided)
    if qname != "bf16":
        assert model.calibration_state()[0]
    return model, d, ts[:steps], lat


# ---- 2. off is off -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_off_is_off(dev, qname):
    model, d, ts, lat = frozen_request(dev, qname, "plain")
    for use_graph in (True, False):
        a = denoise(model, d, ts, img=lat, use_graph=use_graph)
        ws = ws_bytes(model)
        b = denoise(model, d, ts, img=lat, use_graph=use_graph, cache_threshold=0.0, cache_max_hits=3)
        assert torch.equal(a, b) and ws_bytes(model) == ws
        ratios, hits = model.step_cache_log()
        assert ratios.numel() == 0 and hits == []
    # plain -> cached -> plain on ONE engine == each on a fresh engine
    runs = [lambda: denoise(model, d, ts, img=lat), lambda: denoise(model, d, ts, img=lat, cache_threshold=1e30, cache_max_hits=2),
            lambda: denoise(model, d, ts, img=lat)]
    got = [r() for r in runs]
    assert ws_bytes(model) > ws, "the cache buffers are counted once a cached request has run"
    assert torch.equal(got[0], got[2]) and torch.equal(got[0], a) and not torch.equal(got[0], got[1])
    for i, r in enumerate(runs):
        model._invalidate_engine()
        fresh = r()
        assert torch.equal(got[i], fresh), f"request {i} on the shared engine differs from a fresh engine: rel-L2 {rel_l2(got[i], fresh):.3e}"
        if i != 1:
            assert ws_bytes(model) == ws


# ---- 2b. one engine, both graph sets, both update kinds ------------------------------------------------------------------------------------
def _halves(d2):
    return {k: v[:1] for k, v in d2.items()}


@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_cached_plain_and_cached_guided_never_share_graphs(dev, qname):
    """The prepared shape (2 samples) five times on ONE engine -- cached plain B = 2, cached guided B = 1, cached plain B = 2, plain B = 2,
    guided B = 1, 8 frozen steps each -- equals each request on a fresh engine: latents bit for bit, and the hit log."""
    model, d2, ts, lat = frozen_request(dev, qname, "plain")
    d1 = _halves(d2)
    ckw = dict(cache_threshold=1e30, cache_max_hits=2)  # miss, hit, hit, miss, ... whatever the ratios
    runs = [lambda: denoise(model, d2, ts, img=lat, **ckw), lambda: denoise(model, d1, ts, img=lat[:1], guided=True, **ckw),
            lambda: denoise(model, d2, ts, img=lat, **ckw), lambda: denoise(model, d2, ts, img=lat),
            lambda: denoise(model, d1, ts, img=lat[:1], guided=True)]

    def logged(r):
        out = r()
        return out, model.step_cache_log()[1]

    got = [logged(r) for r in runs]
    n = len(ts) - 1
    assert n == 8 and [h for _, h in got] == [[i % 3 != 0 for i in range(n)]] * 3 + [[], []]
    assert torch.equal(got[0][0], got[2][0]), f"requests 1 and 3 differ: rel-L2 {rel_l2(got[0][0], got[2][0]):.3e}"
    for i, r in enumerate(runs):
        model._invalidate_engine()
        fresh, hits = logged(r)
        assert torch.equal(got[i][0], fresh), f"request {i} on the shared engine differs from a fresh engine: rel-L2 {rel_l2(got[i][0], fresh):.3e}"
        assert got[i][1] == hits, f"request {i}: hits {got[i][1]} on the shared engine, {hits} on a fresh one"


@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_single_frozen_step_then_other_update_kind(dev, qname):
    """A request of ONE frozen step leaves its step kind warmed with nothing captured; the next request on the shape has the other update
    kind.  With the cache: guided, then plain; without: plain, then guided.  The second request equals itself on a fresh engine and its
    eager run."""
    model, d2, ts, lat = frozen_request(dev, qname, "plain")
    d1 = _halves(d2)
    ckw = dict(cache_threshold=1e30)
    pairs = {"cached": (lambda: denoise(model, d1, ts[:2], img=lat[:1], guided=True, **ckw), lambda **kw: denoise(model, d2, ts, img=lat, **ckw, **kw)),
             "plain": (lambda: denoise(model, d2, ts[:2], img=lat), lambda **kw: denoise(model, d1, ts, img=lat[:1], guided=True, **kw))}
    for name, (short, long) in pairs.items():
        model._invalidate_engine()
        assert torch.isfinite(short()).all()
        got, hits = long(), model.step_cache_log()[1]
        assert hits == ([False] + [True] * (len(ts) - 2) if name == "cached" else [])
        model._invalidate_engine()
        fresh = long()
        assert torch.equal(got, fresh), f"{name}: behind a one-step request of the other kind vs a fresh engine: rel-L2 {rel_l2(got, fresh):.3e}"
        assert model.step_cache_log()[1] == hits
        eager = long(use_graph=False)
        assert torch.equal(got, eager), f"{name}: graph vs eager: rel-L2 {rel_l2(got, eager):.3e}"
        assert model.step_cache_log()[1] == hits


# ---- 3. extremes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_extremes(dev, qname):
    model, d, ts, lat = frozen_request(dev, qname, "plain")
    n = len(ts) - 1
    plain = denoise(model, d, ts, img=lat)
    every = denoise(model, d, ts, img=lat, cache_threshold=1e30)
    ratios, hits = model.step_cache_log()
    assert hits == [False] + [True] * (n - 1) and tuple(ratios.shape) == (n, 2)
    assert torch.isinf(ratios[0]).all() and torch.isfinite(ratios[1:]).all() and (ratios[1:] > 0).all()
    assert not torch.equal(every, plain) and torch.isfinite(every).all()
    denoise(model, d, ts, img=lat, cache_threshold=1e30, cache_max_hits=2)
    assert model.step_cache_log()[1] == [i % 3 != 0 for i in range(n)], "miss, hit, hit, miss, ..."
    denoise(model, d, ts, img=lat, cache_threshold=1e30, cache_max_hits=1, use_graph=False)
    assert model.step_cache_log()[1] == [i % 2 != 0 for i in range(n)]
    # a threshold below every ratio: no hit, and the latents are the plain run's bit for bit (graph and eager)
    none = denoise(model, d, ts, img=lat, cache_threshold=1e-30)
    ratios, hits = model.step_cache_log()
    assert not any(hits) and ratios[1:].min().item() > 1e-30
    assert torch.equal(none, plain), f"all-miss cached run vs plain: rel-L2 {rel_l2(none, plain):.3e}"
    assert torch.equal(denoise(model, d, ts, img=lat, cache_threshold=1e-30, use_graph=False), plain)
    # refusals of the C entry
    from fluxmi import _lib
    for bad in ((-1.0, 0), (float("nan"), 0), (0.5, -1)):
        with pytest.raises(RuntimeError, match="engine_set_step_cache"):
            _lib.call("fluxmi_engine_set_step_cache", model._engine, bad[0], bad[1])


# ---- 4. graph loop == eager loop == Python loop at a threshold with hits AND misses; 5. what a miss / a hit is ------------------------------
KNOB_SETS = (dict(prefetch=0), dict(prefetch=2), dict(gemm_persist=0), dict(qlut=0), dict(fuse_kv=1), dict(fuse_kv=0), dict(w_pairs=0), dict(a_pairs=0))
CASES = ["plain", "kontext", "fill", "guided"]


def pick_threshold(model, d, ts, lat, guided):
    """From the ratios of an all-miss run: the first of at most three candidates whose cached run has a hit and a miss and keeps every
    decided ratio >= 1 % away from it (the metric errs by 1e-5: three orders of magnitude of clearance).  No candidate: the test fails."""
    denoise(model, d, ts, img=lat, guided=guided, cache_threshold=1e-30)
    base = model.step_cache_log()[0][1:].max(dim=1).values  # per step, the sample that decides
    # candidates: the middles of the widest gaps between the sorted all-miss ratios, those first that the first decided step (whose ratio
    # is on the all-miss path whatever the threshold) stays above: that step then misses and the first step below the threshold hits
    srt = sorted(base.tolist())
    gaps = sorted(((hi - lo, 0.5 * (lo + hi)) for lo, hi in zip(srt[:-1], srt[1:])), key=lambda g: (base[0].item() <= g[1], -g[0]))
    tried = []
    for _, thr in gaps[:3]:
        out = denoise(model, d, ts, img=lat, guided=guided, cache_threshold=thr)
        ratios, hits = model.step_cache_log()
        clear = fu.clearance(ratios.double(), hits, thr)
        tried.append((thr, hits, clear))
        print(f"[fbcache threshold {thr:.5f}] hits {''.join('H' if h else 'm' for h in hits)} clearance {clear:.3f}; all-miss ratios "
              f"{[round(v, 5) for v in base.tolist()]}")
        if any(hits) and not all(hits[1:]) and clear >= 0.01:
            return thr, out, ratios, hits
    pytest.fail(f"no threshold candidate gives a hit and a miss with 1 % clearance: {tried}")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_graph_eager_and_python_loops_agree(dev, qname, case):
    from fluxmi import _lib

    kind, guided = ("plain", True) if case == "guided" else (case, False)
    model, d, ts, lat = frozen_request(dev, qname, kind, B=1, steps=7, guided=guided)  # 6 steps: few enough decided ratios to clear 1 %
    mode = 1 if qname == "fp8" else 2
    thr, a, ratios, hits = pick_threshold(model, d, ts, lat, guided)
    assert a.shape == d["img"].shape and torch.isfinite(a).all()
    # the Python loop on the engine's buffers, right behind the graph run of the same request
    Lt, Lpred = d["txt"].shape[1], d["img"].shape[1]
    stream = model._with_channels(lat, d.get("cond"), d.get("seq"))
    stream, _, Lc = model._with_reference(stream, d["img_ids"], d.get("seq"), d.get("seq_ids"))
    px, pr, ph = fu.python_cached_loop(model, stream.to(torch.bfloat16), ts, mode, thr, 0, Lt, Lpred, scale=SCALE if guided else None)
    assert ph == hits, f"python loop decided {ph}, the engine {hits}"
    assert fu.clearance(pr, ph, thr) >= 0.01
    fin = torch.isfinite(pr)
    assert torch.allclose(pr[fin], ratios.double()[fin], rtol=1e-4, atol=0), "logged fp32 ratios vs fp64 ratios of the Python loop"
    c = px[:, :Lpred, :model.out_channels]
    assert torch.equal(a, c), f"graph loop vs python loop: rel-L2 {rel_l2(a, c):.3e}"
    b = denoise(model, d, ts, img=lat, guided=guided, cache_threshold=thr, use_graph=False)
    assert model.step_cache_log()[1] == hits
    assert torch.equal(a, b), f"graph vs eager: rel-L2 {rel_l2(a, b):.3e}"
    assert not torch.equal(a, denoise(model, d, ts, img=lat, guided=guided)), "the hits changed nothing"
    if qname == "fp8":
        for knobs in KNOB_SETS:
            with _lib.tuning(**knobs):
                a3 = denoise(model, d, ts, img=lat, guided=guided, cache_threshold=thr)
            assert model.step_cache_log()[1] == hits
            assert torch.equal(a, a3), f"cached latents change under tuning {knobs}: rel-L2 {rel_l2(a3, a):.3e}"


@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_what_a_miss_stores_and_a_hit_applies(dev, qname):
    """Behind a request whose LAST step missed, the engine's buffers hold that step: R == bf16(x_final - h1) on the final layer's rows.  Behind
    one whose last step hit: x == bf16(h1 + R) with h1 recomputed through the phase hook, and pred == final_layer of it."""
    model, d, ts, lat = frozen_request(dev, qname, "kontext", steps=8)  # 7 steps
    mode = 1 if qname == "fp8" else 2
    B, Lt, Lpred, H = 2, d["txt"].shape[1], d["img"].shape[1], model.hidden_size
    L = Lt + Lpred + d["seq"].shape[1]
    denoise(model, d, ts, img=lat, cache_threshold=1e30, cache_max_hits=1)  # m H m H m H m
    assert model.step_cache_log()[1][-1] is False
    x = fu.eng_read(model, "x", (B, L, H))[:, Lt:Lt + Lpred]
    h1, R = fu.eng_read(model, "fb_h1", (B, Lpred, H)), fu.eng_read(model, "fb_R", (B, Lpred, H))
    assert torch.equal(R, x - h1) and R.float().abs().sum() > 0
    assert torch.equal(fu.eng_read(model, "fb_rref", (B, Lpred, H)), fu.eng_read(model, "fb_h0", (B, Lpred, H))), "a miss commits r_ref = r"
    out = denoise(model, d, ts[:7], img=lat, cache_threshold=1e30, cache_max_hits=1)  # 6 steps: m H m H m H
    assert model.step_cache_log()[1][-1] is True
    x_hit = fu.eng_read(model, "x", (B, L, H))
    R = fu.eng_read(model, "fb_R", (B, Lpred, H))
    pred = fu.eng_read(model, "pred_s", (B, Lpred, 64))
    # the last step's head again, by hand: the stream before that step is out - dt * pred, which the update cannot be inverted for bit
    # for bit -- so take it from a 5-step run of the same request
    before = denoise(model, d, ts[:6], img=lat, cache_threshold=1e30, cache_max_hits=1)
    stream, _, _ = model._with_reference(before, d["img_ids"], d["seq"], d["seq_ids"])
    denoise(model, d, ts[:7], img=lat, cache_threshold=1e30, cache_max_hits=1)  # the table and the text of the 6-step request again
    with model._lock:
        fu.eng_write(model, "img_s", stream)
        fu.run_phase(model, mode, 0, 1, step=5)
        xs = fu.eng_read(model, "x", (B, L, H))
        xs[:, Lt:Lt + Lpred] = xs[:, Lt:Lt + Lpred] + R
        assert torch.equal(xs[:, Lt:Lt + Lpred], x_hit[:, Lt:Lt + Lpred]), "a hit leaves x = bf16(h1 + R)"
        fu.eng_write(model, "x", xs)
        fu.run_phase(model, mode, 3, 3)
        assert torch.equal(fu.eng_read(model, "pred_s", (B, Lpred, 64)), pred)
    assert torch.equal(out, before + (ts[6] - ts[5]) * pred)


# ---- 6. against the oracle -----------------------------------------------------------------------------------------------------------------
def oracle_cached_loop(o, inp, ts, hits, guidance=3.5, attn_fn=None):
    """fo.denoise with the rule composed from the oracle's own blocks and FORCED to a hit pattern (one entry per step), so that no decision
    can differ from the engine's: a hit step runs the embedders, double block 0 and final_layer(h1 + R), R from the last full step.
    attn_fn: the blocks' attention (fo.attention_exact for the floor) -- passed down, never patched into the module: the full-geometry
    cases' background oracle workers read fo.attention while this test runs"""
    x = inp["img"]
    B, Lt = x.shape[0], inp["txt"].shape[1]
    g = torch.full((B,), guidance, dtype=o.dtype)
    pe = fo.rope_table(torch.cat((inp["txt_ids"], inp["img_ids"]), dim=1), o.p.axes_dim, o.p.theta, o.dtype)
    R = None
    for hit, t_curr, t_prev in zip(hits, ts[:-1], ts[1:]):
        tv = torch.full((B,), t_curr, dtype=o.dtype)
        img = o.lin["img_in"](x)
        vec = o.embed_vec(tv, inp["y"], g)
        txt = o.lin["txt_in"](inp["txt"])
        img, txt = o.double_block(0, img, txt, vec, pe, attn_fn=attn_fn)
        if hit:
            img = img + R
        else:
            h1 = img
            for i in range(1, o.p.depth):
                img, txt = o.double_block(i, img, txt, vec, pe, attn_fn=attn_fn)
            cat = torch.cat((txt, img), 1)
            for i in range(o.p.depth_single_blocks):
                cat = o.single_block(i, cat, vec, pe, attn_fn=attn_fn)
            img = cat[:, Lt:]
            R = img - h1
        x = x + (t_prev - t_curr) * o.final_layer(img, vec)
    return x


def test_cached_denoise_matches_oracle(dev):
    """B = 1, 64 x 64, Lt 32, 20 steps through calibration, threshold 1e30 with at most 2 hits in a row (miss, hit, hit, ... over the frozen
    steps); the oracle loop is forced to the engine's logged pattern.
    fp8 flow: rel-L2(engine, oracle-bf16) <= 1.25 x rel-L2(oracle-fp8, oracle-bf16), all three under that pattern -- gate (iv).
    bf16 flow: rel-L2(engine, oracle-bf16) <= max(1e-2, 1.75 x floor), floor = the oracle's own movement under fo.attention_exact (the gate of
    tests/test_cfg_gpu.py::test_guided_denoise_matches_oracle)."""
    H, W, Lt, n = 64, 64, 32, 20
    ts = fo.get_schedule(n, (H // 16) * (W // 16))
    for qname in ("bf16", "fp8"):
        cfg = tiny_config()
        model, sd = build(cfg, QUANTS[qname], dev)
        inp = inputs("plain", cfg.params, H, W, Lt, 1, seed=7)
        got = denoise(model, to_dev(inp, dev), ts, cache_threshold=1e30, cache_max_hits=2)
        frozen = model.step_cache_log()[1]
        hits = [False] * (n - len(frozen)) + frozen
        assert len(frozen) == (n if qname == "bf16" else n - 13) and frozen == [i % 3 != 0 for i in range(len(frozen))]
        assert torch.isfinite(got).all()
        o16 = oracle_cached_loop(make_oracle(cfg, sd, None), inp, ts, hits)
        e16 = rel_l2(got, o16)
        if qname == "bf16":
            o16x = oracle_cached_loop(make_oracle(cfg, sd, None), inp, ts, hits, attn_fn=fo.attention_exact)
            floor = rel_l2(o16x, o16)
            gate = max(1e-2, 1.75 * floor)
            print(f"[fbcache bf16] engine vs oracle-bf16 {e16:.3e}; floor (oracle-bf16, exact attention) {floor:.3e}; gate {gate:.3e}")
            assert e16 <= gate, f"bf16: rel-L2 {e16:.3e} > max(1e-2, 1.75 x {floor:.3e})"
        else:
            o8 = oracle_cached_loop(make_oracle(cfg, sd, QUANTS[qname]), inp, ts, hits)
            yard = rel_l2(o8, o16)
            print(f"[fbcache fp8] engine vs oracle-bf16 {e16:.3e}; yardstick (oracle-fp8 vs oracle-bf16) {yard:.3e}; ratio {e16 / yard:.3f} (gate 1.25); "
                  f"engine vs oracle-fp8 {rel_l2(got, o8):.3e}")
            assert e16 <= 1.25 * yard, f"fp8: vs bf16 flow {e16:.3e} > 1.25 x {yard:.3e}"


# ---- 7. pipeline ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe(dev):
    p = tiny_pipeline(dev)
    p.compile()
    assert p.model.calibration_state()[0]
    return p


def test_pipeline_cached_request(dev, pipe):
    from PIL import Image

    pos, neg = prompts()
    kw = dict(width=64, height=96, num_steps=8, seed=7, silent=True)
    plain = pipe.generate(pos, output_type="latent", **kw)
    assert pipe.model.step_cache_log()[1] == []
    ckw = dict(cache_threshold=1e30, cache_max_hits=2)
    a = pipe.generate(pos, output_type="latent", **ckw, **kw)
    hits = pipe.model.step_cache_log()[1]
    assert hits == [i % 3 != 0 for i in range(8)]
    assert torch.isfinite(a).all() and a.shape == plain.shape and not torch.equal(a, plain), "a request with hits equals the plain one"
    assert torch.equal(pipe.generate(pos, output_type="latent", cache_threshold=0, **kw), plain)
    assert torch.equal(pipe.generate(pos, output_type="latent", cache_threshold=1e-30, **kw), plain), "an all-miss request differs from the plain one"
    j1, j2 = pipe.generate(pos, **ckw, **kw), pipe.generate(pos, **ckw, **kw)
    assert isinstance(j1, io.BytesIO) and j1.getvalue() == j2.getvalue() and Image.open(j1).size == (64, 96)
    assert j1.getvalue() != pipe.generate(pos, **kw).getvalue()
    for bad in (dict(cache_threshold=-1.0), dict(cache_threshold=float("nan")), dict(cache_threshold=0.5, cache_max_hits=-1)):
        with pytest.raises(ValueError, match="cache_threshold|cache_max_hits"):
            pipe.generate(pos, **bad, **kw)
    # composes with a negative prompt (one decision for both branches), an interval (three calls, each starting empty) and img2img
    g = pipe.generate(pos, negative_prompt=neg, true_cfg_scale=SCALE, output_type="latent", **ckw, **kw)
    ratios, hits = pipe.model.step_cache_log()
    assert hits == [i % 3 != 0 for i in range(8)] and ratios.shape[1] == 2
    assert not torch.equal(g, pipe.generate(pos, negative_prompt=neg, true_cfg_scale=SCALE, output_type="latent", **kw))
    mid = pipe.generate(pos, negative_prompt=neg, true_cfg_scale=SCALE, true_cfg_interval=(0.25, 0.75), output_type="latent", **ckw, **kw)
    assert pipe.model.step_cache_log()[1] == [False, True], "the last of the three calls (2 steps) starts with an empty cache"
    generator, _ = pipe.set_seed(7)
    noise, ts = pipe.preprocess_latent(height=96, width=64, num_steps=8, generator=generator, num_images=1)
    img, img_ids, vec, txt, txt_ids = map(lambda x: x.contiguous(), pipe.prepare(noise, pos))
    _, _, nvec, ntxt, _ = pipe.prepare(noise, neg)
    x = pipe.model.denoise(img, img_ids, txt, txt_ids, vec, ts[0:3], guidance=3.5, **ckw)
    x = pipe.model.denoise(x, img_ids, txt, txt_ids, vec, ts[2:7], guidance=3.5, neg_txt=ntxt, neg_y=nvec, cfg_scale=SCALE, **ckw)
    assert pipe.model.step_cache_log()[1] == [False, True, True, False]
    x = pipe.model.denoise(x, img_ids, txt, txt_ids, vec, ts[6:9], guidance=3.5, **ckw)
    assert torch.equal(mid, pipe.unpack(x.float(), 96, 64))
    import numpy as np

    photo = np.random.default_rng(0).integers(0, 256, size=(96, 64, 3), dtype=np.uint8)
    i2i = pipe.generate(pos, init_image=photo, strength=0.75, output_type="latent", **ckw, **kw)
    n_i2i = len(pipe.model.step_cache_log()[1])
    assert 0 < n_i2i < 8 and torch.isfinite(i2i).all()
    assert not torch.equal(i2i, pipe.generate(pos, init_image=photo, strength=0.75, output_type="latent", **kw))


def test_pipeline_cached_request_composes_with_fill(dev):
    import numpy as np

    p = tiny_pipeline(dev, "fill")
    p.compile()
    pos, _ = prompts()
    photo = np.random.default_rng(0).integers(0, 256, size=(96, 64, 3), dtype=np.uint8)
    mask = np.zeros((96, 64), dtype=np.uint8)
    mask[24:72, 16:48] = 255
    kw = dict(init_image=photo, mask_image=mask, width=64, height=96, num_steps=6, seed=7, silent=True, output_type="latent")
    plain = p.generate(pos, **kw)
    a = p.generate(pos, cache_threshold=1e30, cache_max_hits=1, **kw)
    assert p.model.step_cache_log()[1] == [False, True, False, True, False, True]
    assert a.shape == plain.shape and torch.isfinite(a).all() and not torch.equal(a, plain)
    assert torch.equal(p.generate(pos, cache_threshold=1e-30, **kw), plain)


# ---- 8. real width, once -------------------------------------------------------------------------------------------------------------------
def test_cached_at_1024_real_width(dev):
    """Flux-dev geometry (hidden 3072, 2 + 2 blocks), 1024^2, Lt 512, B 1, fused fp8 flow: graph == eager with hits and misses; the all-miss
    cached run equals the plain run"""
    import util

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    cfg.params.depth, cfg.params.depth_single_blocks = 2, 2
    model, _ = build(cfg, QUANTS["fp8"], dev, seed=2)
    d = to_dev(inputs("plain", cfg.params, 1024, 1024, 512, 1, seed=8, real_tokens=64), dev)
    Li = d["img"].shape[1]
    assert Li + 512 == 4608
    ts = fo.get_schedule(16, Li)
    lat = denoise(model, d, ts[:14], use_graph=False)
    assert model.calibration_state()[0] and torch.isfinite(lat).all()
    ts2 = ts[:8]
    plain = denoise(model, d, ts2, img=lat)
    none = denoise(model, d, ts2, img=lat, cache_threshold=1e-30)
    assert not any(model.step_cache_log()[1])
    assert torch.equal(none, plain), f"all-miss cached run vs plain: rel-L2 {rel_l2(none, plain):.3e}"
    thr, a, ratios, hits = pick_threshold(model, d, ts2, lat, False)
    b = denoise(model, d, ts2, img=lat, cache_threshold=thr, use_graph=False)
    assert model.step_cache_log()[1] == hits
    assert torch.isfinite(a).all() and torch.equal(a, b), f"graph vs eager: rel-L2 {rel_l2(a, b):.3e}"
    print(f"[cached 1024^2 B=1] threshold {thr:.5f} hits {''.join('H' if h else 'm' for h in hits)}; graph == eager; vs plain rel-L2 {rel_l2(a, plain):.3e}")
