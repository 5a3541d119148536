"""Live previews, progress and cancellation on the GPU (include/fluxmi.h: fluxmi_latent_preview, fluxmi_engine_set_preview).

The kernel is checked against the fp64 definition under the band rule of tests/preview_ref.py; the engine against a Python loop that runs the
model per evaluation and calls ops.latent_preview on that evaluation's (x, pred) -- bit for bit, since both run the one kernel on the same
operands.  Helpers are those of tests/test_cfg_gpu.py and tests/test_guidance_gpu.py."""
import numpy as np
import pytest
import torch

import flux_oracle as fo
import inpaint_util as iu
import preview_ref as pr
import solver_util as su
from test_cfg_gpu import QUANTS, SCALE, build, cond_kw, dup, inputs, prompts, rel_l2, tiny_config, tiny_pipeline, to_dev
from test_guidance_gpu import SHAPINGS, shape_pred

pytestmark = pytest.mark.gpu

DEPTH = 2
GRID = (4, 4)  # the token grid of the 64 x 64 requests below
PROJ = np.concatenate([0.15 * np.random.default_rng(77).standard_normal(48), [0.05, -0.1, 0.02]]).astype(np.float32).tolist()


def bf(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(dev)


# ---- 1. the kernel against the fp64 definition ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("grid", [(1, 1), (1, 3), (3, 2), (5, 7), (16, 16)])
def test_kernel_against_fp64(dev, grid, B, guided):
    """trailing Kontext rows and conditioning channels (and the negative half of x) are NaN: none of them may reach the output"""
    from fluxmi import _lib, ops

    n = grid[0] * grid[1]
    x, pred, proj, t, s = pr.draws(B, grid, seed=100 * n + B, guided=guided, img_rows=n + 5, c_in=64 + 16)
    x[:, n:, :] = np.nan
    x[:, :, 64:] = np.nan
    if guided:
        x[B:] = np.nan
    scale = s if guided else None
    want, y, delta = pr.reference_fp64(x, pred, t, proj, grid, scale)
    share = float(pr.in_band(y, delta).mean())
    assert share <= 0.01, f"{share:.4f} of the reference's pixels lie inside the band"
    out = ops.latent_preview(bf(x, dev), bf(pred, dev), float(t), proj.tolist(), grid, scale=None if scale is None else float(scale))
    assert out.shape == (_lib.PREVIEW_SLOTS, B, 2 * grid[0], 2 * grid[1], 3) and out.dtype == torch.uint8
    got = out.cpu().numpy()
    print(f"grid {grid} B {B} guided {guided}: band share {share:.5f}, differing pixels {(got[0] != want).sum()} of {want.size}")
    pr.check_band(got[0], want, y, delta, "kernel")
    assert not got[1:].any(), "a slot other than the selected one was written"


def test_kernel_clamps_and_nan(dev):
    from fluxmi import ops

    grid, B = (5, 7), 2
    x, pred, proj, t, s = pr.draws(B, grid, seed=3, guided=True, amp=8.0)
    x[0, 4, 8:12] = np.nan
    pred[1, 9, 63] = np.inf
    pred[B + 1, 3, 0] = np.nan  # the negative branch of image 1, token 3, channel 0, sub-pixel 0
    want, y, delta = pr.reference_fp64(x, pred, t, proj, grid, s)
    assert (want == 0).mean() > 0.1 and (want == 255).mean() > 0.1
    got = ops.latent_preview(bf(x, dev), bf(pred, dev), float(t), proj.tolist(), grid, scale=float(s))[0].cpu().numpy()
    pr.check_band(got, want, y, delta, "clamped")
    ty, tx = divmod(4, 7)
    assert (got[0, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2] == 0).all(), "NaN maps to 0"
    ty, tx = divmod(3, 7)
    assert (got[1, 2 * ty, 2 * tx] == 0).all()


@pytest.mark.parametrize("every", [1, 3])
def test_cadence_and_slots(dev, every):
    """g = eval_offset + step: skipped evaluations write nothing, written ones land in slot (g / every) % SLOTS"""
    from fluxmi import _lib, ops

    grid, B, off = (3, 2), 2, 5
    S = _lib.PREVIEW_SLOTS
    x, pred, proj, _, _ = pr.draws(B, grid, seed=9)
    xt, pt = bf(x, dev), bf(pred, dev)
    ts = torch.linspace(1.0, 0.1, 8, dtype=torch.float32, device=dev)
    ctl = torch.tensor([every, off], dtype=torch.int32, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.full((S, B, 2 * grid[0], 2 * grid[1], 3), 0xAA, dtype=torch.uint8, device=dev)
    wrote = 0
    for j in range(8):
        before = out.clone()
        step.fill_(j)
        ops.latent_preview(xt, pt, ts, proj.tolist(), grid, step=step, ctl=ctl, out=out)
        g = off + j
        if g % every:
            assert torch.equal(out, before), f"evaluation {g} is skipped and wrote"
            continue
        wrote += 1
        slot = (g // every) % S
        want = ops.latent_preview(xt, pt, float(ts[j]), proj.tolist(), grid)[0]
        assert torch.equal(out[slot], want), f"evaluation {g}: slot {slot} does not hold its preview"
        others = [i for i in range(S) if i != slot]
        assert torch.equal(out[others], before[others]), f"evaluation {g} wrote outside slot {slot}"
    assert wrote == len([j for j in range(8) if (off + j) % every == 0]) > 0
    before = out.clone()
    for bad in ([0, 0], [-2, 0]):
        ops.latent_preview(xt, pt, ts, proj.tolist(), grid, step=step, ctl=bad, out=out)
    assert torch.equal(out, before), "every <= 0 writes nothing"


def test_kernel_refusals(dev):
    from fluxmi import ops

    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match="c_out"):
        ops.latent_preview(z(1, 6, 64), z(1, 6, 32), 0.5, PROJ, (3, 2))
    with pytest.raises(RuntimeError, match="token grid"):
        ops.latent_preview(z(1, 6, 64), z(1, 6, 64), 0.5, PROJ, (2, 2))
    with pytest.raises(RuntimeError, match="bad shape"):
        ops.latent_preview(z(1, 4, 64), z(1, 6, 64), 0.5, PROJ, (3, 2))  # fewer stream rows than predicted rows
    with pytest.raises(RuntimeError, match="bad shape"):
        ops.latent_preview(z(1, 6, 68), z(1, 6, 64), 0.5, PROJ, (3, 2))  # rows that are no multiple of 16 bytes
    with pytest.raises(ValueError, match="51"):
        ops.latent_preview(z(1, 6, 64), z(1, 6, 64), 0.5, PROJ[:50], (3, 2))


# ---- 2. the engine ---------------------------------------------------------------------------------------------------------------------
class Collector:
    def __init__(self, cancel_at=None, raise_at=None):
        self.got, self.cancel_at, self.raise_at = [], cancel_at, raise_at

    def __call__(self, evaluation, n_evaluations, rgb):
        self.got.append((evaluation, n_evaluations, rgb))
        if evaluation == self.raise_at:
            raise KeyError("from the callback")
        return evaluation != self.cancel_at

    def previews(self):
        return [p for _, _, p in self.got]


def call(cb, every=1, offset=0, n=0, grid=GRID):
    from modules.flux_model import PreviewCall

    return PreviewCall(PROJ if every > 0 else None, grid, every, offset, n, cb)


def denoise(model, d, ts, img=None, guided=False, **kw):
    if guided:
        kw = dict(kw, neg_txt=d["neg_txt"], neg_y=d["neg_y"], cfg_scale=SCALE)
    return model.denoise(d["img"] if img is None else img, d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts, guidance=3.5, **cond_kw(d), **kw)


def host_loop(model, d, ts, x, mode, guided=False, shaping=None, solver=None, inp=None, grid=GRID):
    """model(...) per evaluation, ops.latent_preview on that evaluation's (x, pred) -- behind the shaping ops, where the engine launches it --
    then the update the existing host loops use.  -> (final x, previews uint8 [evaluations][B, 2h, 2w, 3], the last evaluation's (x, pred, t))"""
    from fluxmi import ops

    x = x.to(torch.bfloat16)
    B = x.shape[0]
    n = 2 * B if guided else B
    two = dup if guided else (lambda t: t)
    g = torch.full((n,), 3.5, dtype=torch.bfloat16, device=x.device)
    kw = {k: two(v) for k, v in cond_kw(d).items()}
    txt, y = (torch.cat((d["txt"], d["neg_txt"]), 0), torch.cat((d["y"], d["neg_y"]), 0)) if guided else (d["txt"], d["y"])
    r = torch.zeros(B, x[0].numel(), dtype=torch.float32, device=x.device)
    times = list(solver.times) if solver is not None else list(ts)
    xs, hist = su.new_state(x)
    out, last = [], None
    for j in range(len(times) - 1):
        tv = torch.full((n,), times[j], dtype=torch.bfloat16, device=x.device)
        pred = model(two(x), two(d["img_ids"]), txt, two(d["txt_ids"]), tv, y, g, mode=mode, **kw).contiguous()
        if shaping is not None:
            pred = shape_pred(pred, r, shaping, SCALE, j)
        out.append(ops.latent_preview(two(x).contiguous(), pred, float(times[j]), PROJ, grid, scale=SCALE if guided else None)[0].cpu().numpy())
        last = (x.clone(), pred.clone(), float(times[j]))
        v = (pred[:B], pred[B:]) if guided else pred
        dt = times[j + 1] - times[j]
        if solver is not None:
            x = su.apply_row(x, v, solver.coef[j], solver.ctl[j], xs, hist, scale=SCALE if guided else None)
        elif inp is not None:
            x = iu.blend_step(x, v, dt, times[j + 1], inp[0], inp[1], inp[2], scale=SCALE if guided else None)
        elif guided:
            x = x + dt * (v[1] + SCALE * (v[0] - v[1]))
        else:
            x = x + dt * pred
    return x, out, last


def same(a, b, what):
    assert len(a) == len(b), f"{what}: {len(a)} previews vs {len(b)}"
    for j, (p, q) in enumerate(zip(a, b)):
        assert p is not None and p.shape == q.shape and p.dtype == np.uint8, f"{what}: evaluation {j}"
        assert np.array_equal(p, q), f"{what}: evaluation {j} differs in {(p != q).sum()} of {p.size} bytes (max {np.abs(p.astype(int) - q).max()})"


@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_previews_through_calibration_and_replay(dev, qname):
    """a fresh model's first request: fp8 runs 13 calibrating evaluations, one eager frozen one, then replays; every one delivers its preview"""
    cfg = tiny_config()
    model, _ = build(cfg, QUANTS[qname], dev)
    ref, _ = build(cfg, QUANTS[qname], dev)  # the same weights: the host loop's own model, calibrated by its own forwards
    d = to_dev(inputs("plain", cfg.params, 64, 64, 32, 2, seed=5), dev)
    ts = fo.get_schedule(16, d["img"].shape[1])
    cb = Collector()
    lat = denoise(model, d, ts, preview=call(cb, n=16))
    want, pv, last = host_loop(ref, d, ts, d["img"].clone(), None)
    assert [(e, n) for e, n, _ in cb.got] == [(j, 16) for j in range(16)]
    assert torch.equal(lat, want), f"latents: engine vs host loop rel-L2 {rel_l2(lat, want):.3e}"
    same(cb.previews(), pv, "through calibration")
    assert len({p.tobytes() for p in pv}) == 16 and all(p.shape == (2, 8, 8, 3) for p in pv)
    if qname == "fp8":
        assert model.calibration_state()[0]
    # the last evaluation of a schedule that ends at 0 previews the returned latent, up to the bf16 roundings of the update
    # x' = bf16(x + bf16(dt v)): |x' - x0| <= 2^-8 (|dt v| + |x'|) per element, times |M| and 127.5 levels, plus the two rints
    from fluxmi import ops

    assert ts[-1] == 0.0
    of_latent = ops.latent_preview(lat, torch.zeros_like(lat), 0.0, PROJ, GRID)[0].cpu().numpy().astype(int)
    xl, pl, tl = last
    err = 2.0 ** -8 * ((tl * pl.double()).abs() + lat.double().abs()).cpu().numpy().reshape(2, 16, 16, 4)
    M = np.abs(np.asarray(PROJ[:48], np.float64).reshape(16, 3))
    bound = pr._to_image(127.5 * np.einsum("bncs,ck->bnsk", err, M), 2, *GRID) + 1.0
    diff = np.abs(of_latent - cb.previews()[-1].astype(int))
    print(f"{qname}: last preview vs projected latent: max |d| {diff.max()}, max bound {bound.max():.2f}")
    assert (diff <= bound).all() and bound.max() < 12, f"last preview vs projected latent: {diff.max()} levels, bound {bound.max():.2f}"


@pytest.fixture(scope="module")
def frozen(dev):
    """one calibrated fp8 model, a 2-image request and a latent part-way down the schedule, shared by the tests below (none changes them)"""
    cfg = tiny_config()
    model, _ = build(cfg, QUANTS["fp8"], dev)
    d = to_dev(inputs("plain", cfg.params, 64, 64, 32, 2, seed=5), dev)
    ts = fo.get_schedule(16, d["img"].shape[1])
    lat = denoise(model, d, ts[:14], use_graph=False)
    assert model.calibration_state()[0]
    return cfg, model, d, ts, lat


CASES = {
    "plain": dict(),
    "guided": dict(guided=True),
    "shaped": dict(guided=True, shaping="apg"),
    "heun": dict(solver="heun"),
    "blend": dict(inp=True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_previews_bit_exact_and_latents_unchanged(dev, frozen, case):
    """graph == eager == the Python loop for the previews; the latents are those of the request without previews, and with a hook only"""
    from fluxmi import solvers

    cfg, model, d, ts, lat = frozen
    c = CASES[case]
    ts2 = ts[8:13]
    guided = c.get("guided", False)
    kw, hkw = dict(guided=guided), dict(guided=guided)
    if "shaping" in c:
        kw["guidance_shaping"] = hkw["shaping"] = SHAPINGS[c["shaping"]]
    if "solver" in c:
        kw["solver"] = hkw["solver"] = solvers.build_program(c["solver"], ts2)
    if "inp" in c:
        inp = iu.make_inpaint(2, d["img"].shape[1], 64, 5, device=dev)
        kw.update(inpaint_x0=inp[0], inpaint_noise=inp[1], inpaint_mask=inp[2])
        hkw["inp"] = inp
    n = len(kw["solver"].coef) if "solver" in kw else len(ts2) - 1
    base = denoise(model, d, ts2, img=lat, **kw)
    want, pv, _ = host_loop(model, d, ts2, lat.clone(), 1, **hkw)
    assert torch.equal(base, want), f"{case}: the request without previews differs from the host loop: rel-L2 {rel_l2(base, want):.3e}"
    g, e, h = Collector(), Collector(), Collector()
    a = denoise(model, d, ts2, img=lat, preview=call(g, n=n), **kw)
    b = denoise(model, d, ts2, img=lat, preview=call(e, n=n), use_graph=False, **kw)
    o = denoise(model, d, ts2, img=lat, preview=call(h, every=0, n=n), **kw)
    assert torch.equal(a, base) and torch.equal(b, base) and torch.equal(o, base), f"{case}: previews or the hook changed the latents"
    assert torch.equal(denoise(model, d, ts2, img=lat, **kw), base), f"{case}: a request behind previewed ones differs"
    same(g.previews(), pv, f"{case}: graph vs host loop")
    same(e.previews(), pv, f"{case}: eager vs host loop")
    assert [(ev, m) for ev, m, _ in g.got] == [(j, n) for j in range(n)] and len(pv) == n
    assert [(ev, m, p) for ev, m, p in h.got] == [(j, n, None) for j in range(n)], "a hook without previews gets every evaluation and no image"


@pytest.mark.parametrize("kind", ["kontext", "fill"])
def test_previews_read_the_stepped_rows_and_channels(dev, kind):
    """bf16 model (no calibration): Kontext's reference rows and Fill's conditioning channels trail what the preview reads"""
    cfg = tiny_config(kind)
    model, _ = build(cfg, None, dev)
    d = to_dev(inputs(kind, cfg.params, 64, 64, 32, 2, seed=5), dev)
    ts = fo.get_schedule(16, d["img"].shape[1])[9:13]
    for guided in (False, True):
        g = Collector()
        a = denoise(model, d, ts, guided=guided, preview=call(g, n=3))
        want, pv, _ = host_loop(model, d, ts, d["img"].clone(), 2, guided=guided)
        assert torch.equal(a, want)
        same(g.previews(), pv, f"{kind} guided={guided}")


def test_one_graph_for_every_cadence(dev, frozen):
    cfg, model, d, ts, lat = frozen
    ts2 = ts[6:13]
    _, pv, _ = host_loop(model, d, ts2, lat.clone(), 1)
    a = Collector()
    denoise(model, d, ts2, img=lat, preview=call(a, every=1, offset=0, n=6))
    denoise(model, d, ts2, img=lat, preview=call(Collector(), every=1, offset=0, n=6))
    cap = model.preview_stats()[0]
    b = Collector()
    denoise(model, d, ts2, img=lat, preview=call(b, every=3, offset=4, n=20))
    c = Collector()
    denoise(model, d, ts2, img=lat, preview=call(c, every=2, offset=1, n=7))
    assert model.preview_stats()[0] == cap, "another cadence or offset re-captured the step graph"
    same(a.previews(), pv, "every 1")
    assert [(e, n, p is not None) for e, n, p in b.got] == [(4 + j, 20, (4 + j) % 3 == 0) for j in range(6)]
    assert [(e, n, p is not None) for e, n, p in c.got] == [(1 + j, 7, (1 + j) % 2 == 0) for j in range(6)]
    same([p for p in b.previews() if p is not None], [pv[2], pv[5]], "every 3, offset 4")
    same([p for p in c.previews() if p is not None], [pv[1], pv[3], pv[5]], "every 2, offset 1")
    denoise(model, d, ts2, img=lat)
    assert model.preview_stats()[0] == cap + 1, "previewed versus not is a graph kind: the plain request captures its own"


def test_an_images_previews_do_not_depend_on_its_batch(dev):
    cfg = tiny_config()
    model, _ = build(cfg, None, dev)
    d3 = to_dev(inputs("plain", cfg.params, 64, 64, 32, 3, seed=9), dev)
    d1 = {k: v[1:2] for k, v in d3.items()}
    ts = fo.get_schedule(16, d3["img"].shape[1])[8:13]
    for guided in (False, True):
        three, one = Collector(), Collector()
        denoise(model, d3, ts, guided=guided, preview=call(three, n=4))
        denoise(model, d1, ts, guided=guided, preview=call(one, n=4))
        same([p[1:2] for p in three.previews()], one.previews(), f"image 1 of 3 vs alone, guided={guided}")


@pytest.mark.parametrize("k", [0, 2, 5, 7])
def test_cancellation(dev, frozen, k):
    """cancelling at evaluation k: the hook saw 0 .. k, min(n, k + DEPTH) evaluations ran, and the engine is as good as new"""
    from fluxmi import GenerationCancelled

    cfg, model, d, ts, lat = frozen
    ts2, n = ts[4:12], 7
    want = denoise(model, d, ts2, img=lat)
    cb = Collector(cancel_at=k)
    if k >= n:
        assert torch.equal(denoise(model, d, ts2, img=lat, preview=call(cb, n=n)), want)
        return
    with pytest.raises(GenerationCancelled) as ei:
        denoise(model, d, ts2, img=lat, preview=call(cb, n=n))
    assert [e for e, _, _ in cb.got] == list(range(k + 1)), "the hook is called for evaluations 0 .. k only"
    ran = min(n, k + DEPTH)
    assert ei.value.evaluations == ran and ei.value.num_evaluations == n and model.preview_stats()[1] == ran
    a = denoise(model, d, ts2, img=lat)
    g = denoise(model, d, ts2, img=lat, guided=True)
    assert torch.equal(a, want), "the request behind a cancelled one differs"
    model._invalidate_engine()
    assert torch.equal(denoise(model, d, ts2, img=lat), a) and torch.equal(denoise(model, d, ts2, img=lat, guided=True), g), \
        "requests behind a cancelled one differ from a fresh engine's"


def test_cancellation_without_a_graph_and_exceptions(dev, frozen):
    from fluxmi import GenerationCancelled

    cfg, model, d, ts, lat = frozen
    ts2 = ts[4:12]
    want = denoise(model, d, ts2, img=lat)
    cb = Collector(cancel_at=1)
    with pytest.raises(GenerationCancelled) as ei:
        denoise(model, d, ts2, img=lat, use_graph=False, preview=call(cb, every=0, n=7))
    assert ei.value.evaluations == 3 and len(cb.got) == 2
    cb = Collector(raise_at=2)
    with pytest.raises(KeyError, match="from the callback"):
        denoise(model, d, ts2, img=lat, preview=call(cb, n=7))
    assert len(cb.got) == 3 and model.preview_stats()[1] == 4
    assert torch.equal(denoise(model, d, ts2, img=lat), want)


def test_cancellation_in_the_calibrating_steps(dev):
    """the trial counters advance by the calibrating evaluations that ran"""
    from fluxmi import GenerationCancelled

    cfg = tiny_config()
    model, _ = build(cfg, QUANTS["fp8"], dev)
    ref, _ = build(cfg, QUANTS["fp8"], dev)
    d = to_dev(inputs("plain", cfg.params, 64, 64, 32, 1, seed=5), dev)
    ts = fo.get_schedule(16, d["img"].shape[1])
    with pytest.raises(GenerationCancelled) as ei:
        denoise(model, d, ts, preview=call(Collector(cancel_at=3), n=16))
    assert ei.value.evaluations == 5
    denoise(ref, d, ts[:6])  # five evaluations, uncancelled
    assert model.calibration_state() == ref.calibration_state() and model.calibration_state()[1] == 5
    assert torch.equal(denoise(model, d, ts), denoise(ref, d, ts)), "a model cancelled while calibrating continues like one that ran those steps"


def test_step_cached_steps_deliver_previews(dev, frozen):
    cfg, model, d, ts, lat = frozen
    ckw = dict(cache_threshold=1e6, cache_max_hits=1)  # misses and hits alternate: both tails of the cached step run previewed
    base = denoise(model, d, ts[:9], img=lat, **ckw)
    g, e = Collector(), Collector()
    a = denoise(model, d, ts[:9], img=lat, preview=call(g, n=8), **ckw)
    hits = model.step_cache_log()[1]
    b = denoise(model, d, ts[:9], img=lat, use_graph=False, preview=call(e, n=8), **ckw)
    assert any(hits) and not all(hits), hits
    assert torch.equal(a, base) and torch.equal(b, base)
    assert len(g.got) == 8 and all(p is not None for p in g.previews())
    same(g.previews(), e.previews(), "cached: graph vs eager")
    assert len({p.tobytes() for p in g.previews()}) == 8


def test_engine_refusals(dev, frozen):
    cfg, model, d, ts, lat = frozen
    ts2 = ts[8:11]
    with pytest.raises(RuntimeError, match="token grid"):
        denoise(model, d, ts2, img=lat, preview=call(Collector(), grid=(2, 4)))
    model.enable_amax_exchange(reduce_fn=lambda t: None)
    try:
        with pytest.raises(ValueError, match="process group"):
            denoise(model, d, ts2, img=lat, preview=call(Collector()))
    finally:
        model.enable_amax_exchange(reduce_fn=False)
    big = {k: v[:1].expand(33, *v.shape[1:]) for k, v in d.items()}
    with pytest.raises(ValueError, match="one engine pass"):
        denoise(model, big, ts2, preview=call(Collector()))
    want = denoise(model, d, ts2, img=lat)
    g = Collector()
    assert torch.equal(denoise(model, d, ts2, img=lat, preview=call(g, n=2)), want) and len(g.got) == 2


# ---- 3. the pipeline -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe(dev):
    p = tiny_pipeline(dev)
    p.compile()
    assert p.model.calibration_state()[0]
    return p


def test_pipeline_on_step(dev, pipe):
    from fluxmi import GenerationCancelled

    pos, neg = prompts()
    kw = dict(width=64, height=96, num_steps=8, seed=7, silent=True, output_type="latent")
    plain = pipe.generate(pos, **kw)
    seen = []
    got = pipe.generate(pos, on_step=seen.append, preview_every=2, **kw)
    assert torch.equal(got, plain), "on_step / preview_every changed the latents"
    assert [i["evaluation"] for i in seen] == list(range(8)) and all(i["num_evaluations"] == 8 for i in seen)
    assert [i["step"] for i in seen] == list(range(8))
    for i in seen:
        if i["evaluation"] % 2 == 0:
            assert i["preview"].shape == (1, 96 // 8, 64 // 8, 3) and i["preview"].dtype == np.uint8
        else:
            assert i["preview"] is None
    assert len({i["preview"].tobytes() for i in seen if i["preview"] is not None}) == 4
    # the fitted factors are cached, and explicit ones are used as given
    assert pipe._preview_fit is not None and pipe.preview_projection() == pipe.preview_projection()
    grey = []
    pipe.generate(pos, on_step=grey.append, preview_every=4, preview_factors=([[0.0] * 3] * 16, [0.0, 1.0, -1.0]), **kw)
    assert [[np.unique(i["preview"][..., c]).tolist() for c in range(3)] for i in grey if i["preview"] is not None] == [[[128], [255], [0]]] * 2
    # progress only
    seen = []
    assert torch.equal(pipe.generate(pos, on_step=seen.append, **kw), plain) and len(seen) == 8 and all(i["preview"] is None for i in seen)
    # a sampler: evaluations and steps differ
    seen = []
    pipe.generate(pos, on_step=seen.append, preview_every=3, sampler="heun", **kw)
    from fluxmi import solvers

    generator, _ = pipe.set_seed(7)
    _, ts = pipe.preprocess_latent(height=96, width=64, num_steps=8, generator=generator, num_images=1)
    prog = solvers.build_program("heun", ts)
    n = len(prog.coef)
    assert n > 8 and all(i["num_evaluations"] == n for i in seen) and [i["evaluation"] for i in seen] == list(range(n))
    assert [i["step"] for i in seen] == [int(v) for v in prog.step_of_eval] and seen[-1]["step"] == 7
    assert [i["preview"] is not None for i in seen] == [j % 3 == 0 for j in range(n)]
    # a request cut into three denoise calls continues its numbering
    gkw = dict(negative_prompt=neg, true_cfg_scale=SCALE, true_cfg_interval=(0.25, 0.75))
    mid = pipe.generate(pos, **gkw, **kw)
    seen = []
    assert torch.equal(pipe.generate(pos, on_step=seen.append, preview_every=2, **gkw, **kw), mid)
    assert [(i["evaluation"], i["num_evaluations"], i["step"], i["preview"] is not None) for i in seen] == [(j, 8, j, j % 2 == 0) for j in range(8)]
    # cancel: across the cut (evaluation 3 is in the guided slice; two more run)
    seen = []
    with pytest.raises(GenerationCancelled) as ei:
        pipe.generate(pos, on_step=lambda i: seen.append(i) or i["evaluation"] != 3, preview_every=2, **gkw, **kw)
    assert len(seen) == 4 and ei.value.evaluations == 5 and ei.value.num_evaluations == 8
    with pytest.raises(ZeroDivisionError):
        pipe.generate(pos, on_step=lambda i: 1 // 0, **kw)
    assert torch.equal(pipe.generate(pos, **kw), plain)
