"""Guidance shaping of true classifier-free guidance on the GPU (csrc/guidance.hip): CFG rescale, APG, CFG-Zero*.

Two launches in front of the guided update: fluxmi_guidance_moments (per-workgroup partials of nine per-image sums, fixed order) and
fluxmi_guidance_combine (fp64 coefficients per image, then v = bf16((alpha c + beta u) + gamma r) written to BOTH halves of pred, so that
every guided update kernel steps with v as it is).  The kernels are compared with tests/guidance_ref.py (fp64, the vector definitions and
the closed-form coefficients), bit for bit with torch fp32 expressions where the arithmetic is pinned, and the engine with a Python loop of
model forward + the two ops + the update.  Model helpers are those of tests/test_cfg_gpu.py."""
import numpy as np
import pytest
import torch

import flux_oracle as fo
import guidance_ref as gr
import inpaint_util as iu
import solver_util as su
from test_cfg_gpu import QUANTS, SCALE, build, cond_kw, dup, inputs, make_oracle, prompts, rel_l2, tiny_config, tiny_pipeline, to_dev

pytestmark = pytest.mark.gpu

# one vector | exactly one workgroup | a one-vector tail workgroup | a ragged second workgroup | three workgroups
SIZES = (8, 16384, 16392, 20480, 40960 + 8)
NAN = float("nan")
U24 = 2.0 ** -24
# the shaping cases of the kernel tests: every mode, with and without rescale / momentum / the clip; evaluation = step + offset
CASES = {
    "cfg": (dict(s=3.5), 0, 0),
    "cfg_rescale": (dict(s=5.0, phi=0.7), 0, 0),
    "apg": (dict(s=4.0, mode="apg", eta=0.25), 0, 0),
    "apg_clip_momentum": (dict(s=6.0, mode="apg", eta=0.5, rho=5.0, mu=-0.5), 3, 0),
    "apg_momentum_rescale": (dict(s=6.0, mode="apg", eta=0.0, rho=50.0, mu=-0.75, phi=0.4), 0, 2),
    "zero_star": (dict(s=3.0, mode="cfg_zero_star"), 0, 0),
    "zero_star_rescale": (dict(s=7.0, mode="cfg_zero_star", phi=1.0), 1, 1),
    "zero_init_below": (dict(s=3.0, mode="cfg_zero_star", phi=0.5, zero_init=3), 1, 1),       # 2 < 3: zeroed
    "zero_init_boundary": (dict(s=3.0, mode="cfg_zero_star", phi=0.5, zero_init=3), 2, 1),    # 3 < 3 is false: shaped
    "zero_init_momentum": (dict(s=4.0, mode="apg", mu=-0.5, zero_init=1), 0, 0),              # zeroed, r still advances
}


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def draws(B, N, seed, dev):
    """pred bf16 [2B, N] with a non-zero mean on c, u = 0.6 c + noise, and r fp32 [B, N] of comparable size: var_p, dd and cc far from 0"""
    g = torch.Generator().manual_seed(seed)
    c = (0.3 + torch.randn(B, N, generator=g)).to(torch.bfloat16)
    u = (0.6 * c.float() + 0.5 * torch.randn(B, N, generator=g)).to(torch.bfloat16)
    r = 0.8 * torch.randn(B, N, generator=g)
    return torch.cat((c, u), 0).contiguous().to(dev), r.contiguous().to(dev)


def f64(t):
    return t.detach().cpu().to(torch.float64).numpy()


def part_sums(part):
    """the partials added in fp64 in ascending g, as the combine stage adds them -> [B, 9]"""
    p = f64(part)
    s = np.zeros((p.shape[0], 9))
    for g in range(p.shape[1]):
        s = s + p[:, g]
    return s


def ulps(got, want64):
    """|got - fp32(want)| in units of fp32(want)'s spacing"""
    w = np.float32(want64)
    return abs(float(np.float32(got)) - float(w)) / float(np.spacing(np.abs(w)) if w != 0 else np.float32(1e-45))


def run_kernels(pred, r, case, moments_r=True):
    """moments + combine on a clone of pred / r -> (v both halves, r after, coef_out, part)"""
    from fluxmi import ops

    kw, step, off = CASES[case] if isinstance(case, str) else case
    v, r2 = pred.clone(), None if r is None else r.clone()
    part = ops.guidance_moments(v, r2 if moments_r else None)
    coef = ops.guidance_combine(v, part, gr.as_params(**kw), r=r2, step=step, step_offset=off)
    torch.cuda.synchronize()
    return v, r2, coef, part


# ---- 1. moments against fp64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_r", [False, True], ids=["no_r", "r"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", SIZES)
def test_moments_against_fp64(dev, N, B, with_r):
    """Per sum |S - S64| <= (64 + 8 + 1) 2^-24 sum |term| with the partials added in fp64: a thread's chain is 64 sequential adds (8 vectors of
    8 elements, guidance_moments_kernel), the tree over the 256 threads has 8 levels (6 butterfly levels in a wave, then (w0 + w1) +
    (w2 + w3)), and each term is one rounded product -- the kernel's chain is the one the bound was stated for."""
    from fluxmi import ops

    pred, r = draws(B, N, 100 + N % 97 + B, dev)
    r = r if with_r else None
    part = ops.guidance_moments(pred, r)
    torch.cuda.synchronize()
    G = -(-N // 16384)
    assert tuple(part.shape) == (B, G, 9) and torch.isfinite(part).all()
    got = part_sums(part)
    for b in range(B):
        c, u, rb = f64(pred[b]), f64(pred[B + b]), None if r is None else f64(r[b])
        want, scale = gr.moments(c, u, rb), gr.abs_moments(c, u, rb)
        for i, name in enumerate(gr.SUMS):
            err, bound = abs(got[b, i] - want[i]), 73 * U24 * scale[i]
            assert err <= bound, f"N={N} B={B} image {b} {name}: |S - S64| = {err:.3e} > {bound:.3e}"
        if r is None:
            assert not part[b, :, [2, 5, 7, 8]].any(), "r == NULL: its sums are 0"
    # batch invariance and determinism: image 2 of a batch of 3 == the same image alone == a second launch, bit for bit
    if B == 3:
        alone = torch.cat((pred[2:3], pred[5:6]), 0).contiguous()
        pa = ops.guidance_moments(alone, None if r is None else r[2:3].contiguous())
        again = ops.guidance_moments(pred, r)
        torch.cuda.synchronize()
        assert torch.equal(bits(pa[0]), bits(part[2])), "an image's partials depend on its batch"
        assert torch.equal(bits(again), bits(part)), "two launches differ"


# ---- 2. the coefficient stage: fp64 formulas on the kernel's own partials ----------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("N", SIZES)
def test_coefficients_within_one_ulp(dev, N, case):
    """coef_out against guidance_ref.coefficients on the kernel's own partials (their error is test 1's): <= 1 fp32 ulp"""
    B = 3
    pred, r = draws(B, N, 200 + N % 89, dev)
    kw, step, off = CASES[case]
    _, _, coef, part = run_kernels(pred, r, case)
    S = part_sums(part)
    prm = gr.as_params(**kw)
    for b in range(B):
        want = gr.coefficients(S[b], N, prm, evaluation=step + off)
        for i, name in enumerate(("alpha", "beta", "gamma", "f")):
            assert ulps(coef[b, i].item(), want[i]) <= 1.0, f"{case} N={N} image {b} {name}: {coef[b, i].item()!r} vs {want[i]!r}"
        if "zero_init_below" in case or case == "zero_init_momentum":
            assert not coef[b, :3].any()
        else:
            assert coef[b, 0] != 0


def test_degenerate_inputs_take_the_fallbacks(dev):
    """c == u and u == 0, run for their fallbacks (dd = 0: tau = 1; uu = 0: s* = 1; var_p = 0: f = 1): finite coefficients, the stated values"""
    N, B = 16392, 1
    pred, _ = draws(B, N, 7, dev)
    same = torch.cat((pred[:B], pred[:B]), 0).contiguous()
    zero_u = torch.cat((pred[:B], torch.zeros_like(pred[:B])), 0).contiguous()
    zeros = torch.zeros_like(pred)
    v, _, coef, _ = run_kernels(same, None, (dict(s=4.0, mode="apg", eta=0.3, rho=1.0, phi=0.5), 0, 0))
    assert torch.isfinite(coef).all() and torch.equal(v[:B], same[:B]) and coef[0, 3] == 1.0, "c == u: p = c, f = 1"
    v, _, coef, _ = run_kernels(zero_u, None, (dict(s=3.0, mode="cfg_zero_star"), 0, 0))
    assert coef[0].tolist() == [3.0, -2.0, 0.0, 1.0]
    for mode in gr.MODES:
        v, _, coef, _ = run_kernels(zeros, None, (dict(s=3.0, mode=mode, phi=0.7, rho=1.0), 0, 0))
        assert torch.isfinite(coef).all() and coef[0, 3] == 1.0 and not v.any(), mode


# ---- 3. combine, bit for bit ----------------------------------------------------------------------------------------------------------------
def torch_combine(pred, r, coef, mu):
    """the torch fp32 expressions of the combine stage with the kernel's coefficients, on the host: torch.mul / torch.add are separate
    operations, one rounding each; a term whose coefficient is 0 is absent -> (v bf16 [B, N], r' fp32 or None)"""
    B = pred.shape[0] // 2
    c, u = pred[:B].float().cpu(), pred[B:].float().cpu()
    rr = None if r is None else r.cpu()
    co = coef.cpu()
    out = []
    for b in range(B):
        al, be, ga = (co[b, i] for i in range(3))
        acc = None
        for k, t in ((al, c[b]), (be, u[b]), (ga, None if rr is None else rr[b])):
            if k != 0 and t is not None:
                term = torch.mul(t, k)
                acc = term if acc is None else torch.add(acc, term)
        out.append((torch.zeros_like(c[b]) if acc is None else acc).to(torch.bfloat16))
    r_new = None
    if mu != 0 and rr is not None:
        r_new = torch.add(torch.sub(c, u), torch.mul(rr, torch.tensor(mu, dtype=torch.float64).to(torch.float32)))
    return torch.stack(out), r_new


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", SIZES)
def test_combine_bit_exact(dev, N, B, case):
    pred, r = draws(B, N, 300 + N % 83 + B, dev)
    kw, _, _ = CASES[case]
    mu = gr.as_params(**kw)[4]
    if mu == 0:
        # an unread r (mu == 0; gamma == 0 follows) may hold anything: poisoned, and left as it was.  The moments see no r.
        poison = torch.full_like(r, NAN)
        v, r2, coef, _ = run_kernels(pred, poison, case, moments_r=False)
        assert torch.equal(bits(r2), bits(poison)), f"{case}: an unread r was written"
        want, _ = torch_combine(pred, None, coef, 0.0)
    else:
        v, r2, coef, _ = run_kernels(pred, r, case)
        want, r_want = torch_combine(pred, r, coef, mu)
        assert torch.equal(bits(r2.cpu()), bits(r_want)), f"{case} N={N} B={B}: r' differs"
    assert torch.isfinite(v).all()
    assert torch.equal(v[:B].cpu(), want), f"{case} N={N} B={B}: rel-L2 {rel_l2(v[:B], want):.3e}"
    assert torch.equal(bits(v[B:]), bits(v[:B])), "the halves differ"
    if "zero_init" in case and "boundary" not in case:
        assert not v.any()
    # r == NULL altogether: mu counts as 0 whatever params says
    if mu != 0:
        v0, _, coef0, _ = run_kernels(pred, None, case)
        want0, _ = torch_combine(pred, None, coef0, 0.0)
        assert torch.equal(v0[:B].cpu(), want0) and not coef0[:, 2].any()


# ---- 4. end to end against the vector reference -------------------------------------------------------------------------------------------
E2E = {}


@pytest.mark.parametrize("case", [c for c in CASES if "zero_init" not in c])
def test_end_to_end_against_the_vector_reference(dev, case):
    """rel-L2(v, p64) <= 1.25 x rel-L2(bf16(p64), p64) per image, p64 = guidance_ref.shape_vector in float64 from the vector definitions: the
    coefficient error (about 1e-5 relative at most, test 1's bound through the formulas) is below 1 % of the output's bf16 rounding."""
    worst = 0.0
    for N in SIZES:
        B = 3
        pred, r = draws(B, N, 400 + N % 79, dev)
        kw, step, off = CASES[case]
        prm = gr.as_params(**kw)
        v, r2, _, _ = run_kernels(pred, r, case)
        for b in range(B):
            p64, r64, _ = gr.shape_vector(f64(pred[b]), f64(pred[B + b]), f64(r[b]), prm, evaluation=step + off)
            p64t = torch.from_numpy(p64)
            floor = ((p64t.to(torch.bfloat16).to(torch.float64) - p64t).norm() / p64t.norm()).item()
            err = ((v[b].cpu().to(torch.float64) - p64t).norm() / p64t.norm()).item()
            ratio = err / floor
            worst = max(worst, ratio)
            print(f"[guidance e2e {case} N={N} image {b}] rel-L2 vs p64 {err:.4e}; bf16 floor {floor:.4e}; ratio {ratio:.4f} (gate 1.25)")
            assert err <= 1.25 * floor, f"{case} N={N} image {b}: {err:.4e} > 1.25 x {floor:.4e}"
            if r64 is not None:
                e_r = np.abs(f64(r2[b]) - r64).max() / np.abs(r64).max()
                assert e_r <= 4 * U24, f"{case}: r' off by {e_r:.3e}"
    E2E[case] = worst
    print(f"[guidance e2e {case}] worst ratio over sizes and images {worst:.4f}")


# ---- 5. the in-place trick: the guided update kernels step with v unchanged ----------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_guided_updates_step_with_v(dev, B):
    from fluxmi import _lib, ops

    rows, C = 257, 64
    N = rows * C
    pred, r = draws(B, N, 500 + B, dev)
    v, _, _, _ = run_kernels(pred, r, "apg_clip_momentum")
    v = v.view(2 * B, rows, C)
    assert torch.equal(v[:B], v[B:])
    g = torch.Generator().manual_seed(3)
    dts = torch.tensor([-0.0625, 0.0471], dtype=torch.float32, device=dev)
    step = torch.tensor([1], dtype=torch.int32, device=dev)
    coef = torch.tensor([[0.75, 0.3, -0.0625, 0.41, -0.17, 0.9, -0.6, 0.0]] * 2, dtype=torch.float32, device=dev)
    ctl = torch.tensor([[1, 1, 0, 1]] * 2, dtype=torch.int32, device=dev)
    for scale in (0.0, 1.0, 3.5, 7.5):
        sc = torch.tensor([scale], dtype=torch.float32, device=dev)
        img = torch.randn(2 * B, rows, C, generator=g).to(torch.bfloat16).to(dev)
        # fluxmi_cfg_euler on (v, v) == fluxmi_euler on v
        a, b = img.clone(), img[:B].clone().contiguous()
        _lib.call("fluxmi_cfg_euler", ops._p(a), ops._p(v), ops._p(dts), ops._p(step), ops._p(sc), B, rows, rows, C, C, ops._stream())
        _lib.call("fluxmi_euler", ops._p(b), ops._p(v), ops._p(dts), ops._p(step), B * N, ops._stream())
        torch.cuda.synchronize()
        assert torch.equal(bits(a[:B]), bits(b)) and torch.equal(bits(a[B:]), bits(b)), f"cfg_euler at scale {scale} does not step with v"
        # guided fluxmi_solver_step on (v, v) == the unguided one on v: x', the saved iterate and the history slots
        xs0 = torch.randn(B, rows, C, generator=g).to(torch.bfloat16).to(dev)
        h0 = torch.randn(2, B, rows, C, generator=g).to(dev)
        outs = []
        for guided in (True, False):
            x = img.clone() if guided else img[:B].clone().contiguous()
            xs, hist = xs0.clone(), h0.clone()
            _lib.call("fluxmi_solver_step", ops._p(x), ops._p(v), ops._p(xs), ops._p(hist), ops._p(coef), ops._p(ctl), None, None, None, ops._p(dts),
                      ops._p(dts), None, ops._p(step), ops._p(sc) if guided else None, B, rows, rows, C, C, ops._stream())
            torch.cuda.synchronize()
            outs.append((x, xs, hist))
        (xg, xsg, hg), (xp, xsp, hp) = outs
        assert torch.equal(bits(xg[:B]), bits(xp)) and torch.equal(bits(xg[B:]), bits(xp)), f"guided solver_step at scale {scale}"
        assert torch.equal(bits(xsg), bits(xsp)) and torch.equal(bits(hg), bits(hp))


def test_kernel_refusals(dev):
    from fluxmi import _lib, ops

    t = torch.zeros(2, 16, dtype=torch.bfloat16, device=dev)
    part = torch.zeros(1, 1, 9, device=dev)
    prm = torch.zeros(8, device=dev)
    for B, N in ((0, 16), (1, 12), (1, 0), (-1, 16)):
        with pytest.raises(RuntimeError, match="guidance_moments: bad shape"):
            _lib.call("fluxmi_guidance_moments", ops._p(t), None, ops._p(part), B, N, ops._stream())
        with pytest.raises(RuntimeError, match="guidance_combine: bad shape"):
            _lib.call("fluxmi_guidance_combine", ops._p(t), None, ops._p(part), ops._p(prm), None, None, None, B, N, ops._stream())
    with pytest.raises(RuntimeError, match="guidance_moments: NULL argument"):
        _lib.call("fluxmi_guidance_moments", ops._p(t), None, None, 1, 16, ops._stream())
    with pytest.raises(RuntimeError, match="guidance_combine: NULL argument"):
        _lib.call("fluxmi_guidance_combine", ops._p(t), None, ops._p(part), None, None, None, None, 1, 16, ops._stream())
    torch.cuda.synchronize()
    assert not t.any()


# ---- 6. the engine ------------------------------------------------------------------------------------------------------------------------
SHAPINGS = {
    "rescale": dict(rescale=0.7),
    "apg": dict(mode="apg", eta=0.25, norm_threshold=40.0, momentum=-0.5),
    "zero_star": dict(mode="cfg_zero_star", rescale=0.3, zero_init_steps=1),
}


def shaped_denoise(model, d, ts, shaping, img=None, use_graph=True, scale=SCALE, **kw):
    return model.denoise(d["img"] if img is None else img, d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts, guidance=3.5, use_graph=use_graph,
                         neg_txt=d["neg_txt"], neg_y=d["neg_y"], cfg_scale=scale, guidance_shaping=shaping, **cond_kw(d), **kw)


def shape_pred(pred, r, shaping, scale, evaluation):
    """the two ops on the model's prediction [2B, Li, C], in place; r fp32 [B, Li * C]"""
    from fluxmi import ops

    prm = ops.guidance_params(scale, shaping.get("mode", "cfg"), shaping.get("rescale", 0.0), shaping.get("eta", 1.0),
                              shaping.get("norm_threshold", 0.0), shaping.get("momentum", 0.0), shaping.get("zero_init_steps", 0))
    part = ops.guidance_moments(pred, r)
    ops.guidance_combine(pred, part, prm, r=r, step=evaluation, step_offset=shaping.get("step_offset", 0))
    return pred


def python_shaped_loop(model, d, ts, x, mode, shaping, scale=SCALE, inp=None, solver=None):
    """model(cat(x, x)) per evaluation, ops.guidance_moments, ops.guidance_combine, then the guided update: ops.cfg_euler, or the blend /
    solver interpreters of tests/inpaint_util.py / tests/solver_util.py on v (the guided kernels step with v: test 5)"""
    from fluxmi import ops

    B = x.shape[0]
    g = torch.full((2 * B,), 3.5, dtype=torch.bfloat16, device=x.device)
    kw = {k: dup(v) for k, v in cond_kw(d).items()}
    txt, y = torch.cat((d["txt"], d["neg_txt"]), 0), torch.cat((d["y"], d["neg_y"]), 0)
    r = torch.zeros(B, x[0].numel(), dtype=torch.float32, device=x.device)
    times = list(solver.times) if solver is not None else list(ts)
    xs, hist = su.new_state(x)
    for j in range(len(times) - 1):
        tv = torch.full((2 * B,), times[j], dtype=torch.bfloat16, device=x.device)
        pred = model(dup(x), dup(d["img_ids"]), txt, dup(d["txt_ids"]), tv, y, g, mode=mode, **kw).contiguous()
        pred = shape_pred(pred, r, shaping, scale, j)
        if solver is not None:
            x = su.apply_row(x, pred[:B], solver.coef[j], solver.ctl[j], xs, hist)
        elif inp is not None:
            x = iu.blend_step(x, pred[:B], times[j + 1] - times[j], times[j + 1], inp[0], inp[1], inp[2])
        else:
            x = ops.cfg_euler(dup(x).contiguous(), pred, times[j + 1] - times[j], scale)[:B].contiguous()
    return x


@pytest.mark.parametrize("kind", ["plain", "kontext", "fill"])
@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_shaped_denoise_bit_exact(dev, qname, kind):
    """graph == eager == the Python loop, for every mode on one calibrated model; an unshaped guided request is the existing guided loop"""
    from test_cfg_gpu import guided_denoise, python_guided_loop

    cfg = tiny_config(kind)
    model, _ = build(cfg, QUANTS[qname], dev)
    d = to_dev(inputs(kind, cfg.params, 64, 64, 32, 2, seed=5), dev)
    ts = fo.get_schedule(16, d["img"].shape[1])
    lat = shaped_denoise(model, d, ts[:14], SHAPINGS["apg"], use_graph=False)  # fp8: 13 calibrating SHAPED steps, then frozen
    assert lat.shape == d["img"].shape and torch.isfinite(lat).all()
    if qname == "fp8":
        assert model.calibration_state()[0]
    mode = 1 if qname == "fp8" else 2
    ts2 = ts[:7]
    plain = guided_denoise(model, d, ts2, img=lat)
    assert torch.equal(plain, python_guided_loop(model, d, ts2, lat.clone(), mode)), "the unshaped guided request changed"
    outs = {}
    for name, sh in SHAPINGS.items():
        a = shaped_denoise(model, d, ts2, sh, img=lat)
        b = shaped_denoise(model, d, ts2, sh, img=lat, use_graph=False)
        c = python_shaped_loop(model, d, ts2, lat.clone(), mode, sh)
        assert torch.isfinite(a).all() and a.shape == d["img"].shape
        assert torch.equal(a, b), f"{name}: graph vs eager rel-L2 {rel_l2(a, b):.3e}"
        assert torch.equal(a, c), f"{name}: graph loop vs python loop rel-L2 {rel_l2(a, c):.3e}"
        assert not torch.equal(a, plain), f"{name}: no effect"
        outs[name] = a
    assert not torch.equal(outs["apg"], outs["rescale"]) and not torch.equal(outs["apg"], outs["zero_star"])
    assert torch.equal(guided_denoise(model, d, ts2, img=lat), plain), "an unshaped request behind shaped ones differs"


def test_shaping_composes_with_heun_and_the_blend(dev):
    from fluxmi import solvers

    cfg = tiny_config()
    model, _ = build(cfg, QUANTS["fp8"], dev)
    d = to_dev(inputs("plain", cfg.params, 64, 64, 32, 2, seed=5), dev)
    ts = fo.get_schedule(16, d["img"].shape[1])
    lat = shaped_denoise(model, d, ts[:14], SHAPINGS["apg"], use_graph=False)
    assert model.calibration_state()[0]
    ts2 = ts[8:13]
    # heun + APG momentum: one shaping (and one advance of r) per EVALUATION
    prog = solvers.build_program("heun", ts2)
    a = shaped_denoise(model, d, ts2, SHAPINGS["apg"], img=lat, solver=prog)
    b = shaped_denoise(model, d, ts2, SHAPINGS["apg"], img=lat, solver=prog, use_graph=False)
    c = python_shaped_loop(model, d, ts2, lat.clone(), 1, SHAPINGS["apg"], solver=prog)
    assert torch.equal(a, b) and torch.equal(a, c), f"heun + apg: graph vs eager {rel_l2(a, b):.3e}, vs python loop {rel_l2(a, c):.3e}"
    assert not torch.equal(a, shaped_denoise(model, d, ts2, dict(SHAPINGS["apg"], momentum=0.0), img=lat, solver=prog)), "the momentum has no effect"
    # inpaint_mask: the blend kernel behind the shaping
    inp = iu.make_inpaint(2, d["img"].shape[1], 64, 5, device=dev)
    ikw = dict(inpaint_x0=inp[0], inpaint_noise=inp[1], inpaint_mask=inp[2])
    a = shaped_denoise(model, d, ts2, SHAPINGS["zero_star"], img=lat, **ikw)
    b = shaped_denoise(model, d, ts2, SHAPINGS["zero_star"], img=lat, use_graph=False, **ikw)
    c = python_shaped_loop(model, d, ts2, lat.clone(), 1, SHAPINGS["zero_star"], inp=inp)
    assert torch.equal(a, b) and torch.equal(a, c), f"blend + zero*: graph vs eager {rel_l2(a, b):.3e}, vs python loop {rel_l2(a, c):.3e}"
    # step caching is allowed: shaping only touches pred_s (graph == eager with the cache on)
    # (a threshold every finite ratio passes and at most one hit in a row: misses and hits alternate, both tails run shaped)
    ckw = dict(cache_threshold=1e6, cache_max_hits=1)
    a = shaped_denoise(model, d, ts[:9], SHAPINGS["rescale"], img=lat, **ckw)
    hits = model.step_cache_log()[1]
    b = shaped_denoise(model, d, ts[:9], SHAPINGS["rescale"], img=lat, use_graph=False, **ckw)
    assert torch.equal(a, b) and any(hits) and not all(hits), f"cached + shaped: graph vs eager {rel_l2(a, b):.3e}, hits {hits}"


@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_shaped_requests_on_one_engine_equal_fresh_engines(dev, qname):
    """batch invariance (B = 1 vs B = 3), and mode / value changes and shaped / unshaped switches on ONE engine against fresh engines"""
    from test_cfg_gpu import guided_denoise

    cfg = tiny_config()
    model, _ = build(cfg, QUANTS[qname], dev)
    d3 = to_dev(inputs("plain", cfg.params, 64, 64, 32, 3, seed=9), dev)
    d1 = {k: v[1:2] for k, v in d3.items()}
    ts = fo.get_schedule(16, d3["img"].shape[1])
    lat = shaped_denoise(model, d3, ts[:14], SHAPINGS["apg"], use_graph=False)
    ts2 = ts[:7]
    for name, sh in SHAPINGS.items():
        three = shaped_denoise(model, d3, ts2, sh, img=lat)
        one = shaped_denoise(model, d1, ts2, sh, img=lat[1:2])
        assert torch.equal(one[0], three[1]), f"{name}: a shaped sample depends on its batch: rel-L2 {rel_l2(one[0], three[1]):.3e}"
    runs = [lambda: shaped_denoise(model, d1, ts2, SHAPINGS["apg"], img=lat[1:2]),
            lambda: guided_denoise(model, d1, ts2, img=lat[1:2]),
            lambda: shaped_denoise(model, d1, ts2, SHAPINGS["zero_star"], img=lat[1:2]),
            lambda: shaped_denoise(model, d1, ts2, dict(SHAPINGS["apg"], momentum=-0.25, eta=0.0), img=lat[1:2]),
            lambda: shaped_denoise(model, d1, ts2, SHAPINGS["apg"], img=lat[1:2], scale=2.0),
            lambda: guided_denoise(model, d1, ts2, img=lat[1:2]),
            lambda: shaped_denoise(model, d1, ts2, SHAPINGS["apg"], img=lat[1:2])]
    got = [r() for r in runs]
    assert torch.equal(got[0], got[6]) and torch.equal(got[1], got[5]), "a repeated request differs (APG's running difference must restart at 0)"
    assert not torch.equal(got[0], got[3]) and not torch.equal(got[0], got[4])
    for i, r in enumerate(runs):
        model._invalidate_engine()
        fresh = r()
        assert torch.equal(got[i], fresh), f"request {i} on the shared engine differs from a fresh engine: rel-L2 {rel_l2(got[i], fresh):.3e}"


def test_engine_refusals_and_state(dev):
    import ctypes as C

    from fluxmi import _lib, ops

    cfg = tiny_config()
    model, _ = build(cfg, None, dev)
    d2 = to_dev(inputs("plain", cfg.params, 64, 64, 32, 2, seed=2), dev)
    d = {k: v[:1] for k, v in d2.items()}
    ts = fo.get_schedule(4, d["img"].shape[1])
    with pytest.raises(ValueError, match="needs a negative prompt"):
        model.denoise(d["img"], d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts, guidance_shaping=dict(mode="apg"))
    with pytest.raises(ValueError, match="unknown mode"):
        shaped_denoise(model, d, ts, dict(mode="dynamic_thresholding"))
    with pytest.raises(ValueError, match=r"outside \[0, 1\]"):
        shaped_denoise(model, d, ts, dict(rescale=1.25))
    out = shaped_denoise(model, d, ts, SHAPINGS["apg"])
    plain = model.denoise(d2["img"], d2["img_ids"], d2["txt"], d2["txt_ids"], d2["y"], ts)  # the same prepared shape: two samples
    prm = lambda *v: (C.c_float * 8)(*v)
    with model._lock:
        for bad, msg in ((prm(3, 0, 1, 0, 0, 3, 0, 0), "mode"), (prm(3, 1.5, 1, 0, 0, 0, 0, 0), "phi"), (prm(3, 0, 1, -1, 0, 0, 0, 0), "rho"),
                         (prm(3, 0, NAN, 0, 0, 0, 0, 0), "not finite")):
            with pytest.raises(RuntimeError, match=f"engine_set_guidance: .*{msg}"):
                _lib.call("fluxmi_engine_set_guidance", model._engine, bad, 0)
        with pytest.raises(RuntimeError, match="step_offset"):
            _lib.call("fluxmi_engine_set_guidance", model._engine, prm(3, 0, 1, 0, 0, 0, 0, 0), -1)
        # a state left on the engine is not consulted by an unguided call: fluxmi_engine_denoise on the two samples
        _lib.call("fluxmi_engine_set_guidance", model._engine, prm(3, 0.5, 1, 0, 0, 1, 0, 0), 0)
        img, t_io, tsc = d2["img"].clone(), C.c_int(0), (C.c_double * len(ts))(*ts)
        _lib.call("fluxmi_engine_denoise", model._engine, ops._p(img), ops._p(d2["txt"]), ops._p(d2["y"]), 3.5, tsc, len(ts) - 1, C.byref(t_io), 1,
                  ops._stream())
        torch.cuda.synchronize()
        _lib.call("fluxmi_engine_set_guidance", model._engine, None, 0)
    assert torch.equal(img, plain), "an unguided call consulted the shaping state"
    assert torch.equal(out, shaped_denoise(model, d, ts, SHAPINGS["apg"]))


# ---- 7. against the oracle ----------------------------------------------------------------------------------------------------------------
def oracle_shaped_loop(oracle, inp, ts, shaping, scale=SCALE, guidance=3.5):
    """the guided loop on FluxOracle.forward with the shaping applied by guidance_ref in fp32 (shape_vector's float64 result rounded to fp32,
    then to the flow's bf16) and the bf16 Euler update"""
    x = inp["img"]
    B = x.shape[0]
    g = torch.full((2 * B,), guidance, dtype=oracle.dtype)
    txt, y = torch.cat((inp["txt"], inp["neg_txt"]), 0), torch.cat((inp["y"], inp["neg_y"]), 0)
    prm = gr.as_params(scale, shaping.get("mode", "cfg"), shaping.get("rescale", 0.0), shaping.get("eta", 1.0), shaping.get("norm_threshold", 0.0),
                       shaping.get("momentum", 0.0), shaping.get("zero_init_steps", 0))
    r = [np.zeros(x[0].numel()) for _ in range(B)]
    for j, (t_curr, t_prev) in enumerate(zip(ts[:-1], ts[1:])):
        tv = torch.full((2 * B,), t_curr, dtype=oracle.dtype)
        pred = oracle.forward(dup(x), dup(inp["img_ids"]), txt, dup(inp["txt_ids"]), tv, y, g)
        v = []
        for b in range(B):
            p, r_new, _ = gr.shape_vector(f64(pred[b]).ravel(), f64(pred[B + b]).ravel(), r[b], prm, evaluation=j)
            if r_new is not None:
                r[b] = r_new.astype(np.float32).astype(np.float64)
            v.append(torch.from_numpy(p.astype(np.float32)).reshape(pred[b].shape))
        x = x + (t_prev - t_curr) * torch.stack(v).to(x.dtype)
    return x


@pytest.mark.parametrize("name", list(SHAPINGS))
def test_shaped_denoise_matches_oracle(dev, name, monkeypatch):
    """B = 1, 64 x 64, Lt 32, 16 shaped guided steps through calibration; the gate construction of test_guided_denoise_matches_oracle.
    fp8: rel-L2(engine, oracle-bf16 loop) <= 1.25 x rel-L2(oracle-fp8 loop, oracle-bf16 loop) under the same shaping.
    bf16: rel-L2(engine, oracle-bf16) <= max(1e-2, 1.75 x floor), floor = the oracle's own movement with fo.attention_exact."""
    H, W, Lt, B, n = 64, 64, 32, 1, 16
    ts = fo.get_schedule(n, (H // 16) * (W // 16))
    sh = SHAPINGS[name]
    ref = {}
    for qname in ("bf16", "fp8"):
        cfg = tiny_config()
        model, sd = build(cfg, QUANTS[qname], dev)
        inp = inputs("plain", cfg.params, H, W, Lt, B, seed=7)
        if not ref:
            ref["o16"] = oracle_shaped_loop(make_oracle(cfg, sd, None), inp, ts, sh)
            with monkeypatch.context() as mp:
                mp.setattr(fo, "attention", fo.attention_exact)
                ref["floor16"] = rel_l2(oracle_shaped_loop(make_oracle(cfg, sd, None), inp, ts, sh), ref["o16"])
        got = shaped_denoise(model, to_dev(inp, dev), ts, sh)
        assert got.shape == inp["img"].shape and torch.isfinite(got).all()
        e16 = rel_l2(got, ref["o16"])
        if qname == "bf16":
            gate = max(1e-2, 1.75 * ref["floor16"])
            print(f"[guidance {name} bf16] engine vs oracle-bf16 {e16:.3e}; floor (oracle-bf16, exact attention) {ref['floor16']:.3e}; gate {gate:.3e}")
            assert e16 <= gate, f"{name} bf16: rel-L2 {e16:.3e} > max(1e-2, 1.75 x {ref['floor16']:.3e})"
        else:
            yard = rel_l2(oracle_shaped_loop(make_oracle(cfg, sd, QUANTS[qname]), inp, ts, sh), ref["o16"])
            print(f"[guidance {name} fp8] engine vs oracle-bf16 {e16:.3e}; yardstick (oracle-fp8 vs oracle-bf16) {yard:.3e}; ratio {e16 / yard:.3f} (gate 1.25)")
            assert e16 <= 1.25 * yard, f"{name} fp8: vs bf16 flow {e16:.3e} > 1.25 x {yard:.3e}"


# ---- 8. pipeline and HTTP ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe(dev):
    p = tiny_pipeline(dev)
    p.compile()
    assert p.model.calibration_state()[0]
    return p


def test_pipeline_guidance_shaping(dev, pipe):
    pos, neg = prompts()
    kw = dict(width=64, height=96, num_steps=8, seed=7, silent=True, output_type="latent")
    gkw = dict(negative_prompt=neg, true_cfg_scale=SCALE)
    # refusals: any non-default value without guidance, rescale outside [0, 1], an unknown mode
    for bad in (dict(guidance_mode="apg"), dict(guidance_rescale=0.5), dict(zero_init_steps=1), dict(apg_eta=0.5), dict(apg_momentum=-0.5),
                dict(apg_norm_threshold=5.0)):
        with pytest.raises(ValueError, match="need a negative_prompt"):
            pipe.generate(pos, **bad, **kw)
        with pytest.raises(ValueError, match="need a negative_prompt"):
            pipe.generate(pos, negative_prompt=neg, true_cfg_scale=1.0, **bad, **kw)
    for bad, msg in ((dict(guidance_rescale=1.5), "guidance_rescale"), (dict(guidance_rescale=-0.5), "guidance_rescale"),
                     (dict(guidance_mode="dynamic"), "guidance_mode"), (dict(zero_init_steps=-1), "zero_init_steps"),
                     (dict(apg_eta=0.5), "belong to guidance_mode"), (dict(guidance_mode="cfg_zero_star", apg_momentum=-0.5), "belong to guidance_mode")):
        with pytest.raises(ValueError, match=msg):
            pipe.generate(pos, **gkw, **bad, **kw)
    # defaults are today's output, bit for bit: the guided request through Flux.denoise without a shaping state
    full = pipe.generate(pos, **gkw, **kw)
    generator, _ = pipe.set_seed(7)
    noise, ts = pipe.preprocess_latent(height=96, width=64, num_steps=8, generator=generator, num_images=1)
    img, img_ids, vec, txt, txt_ids = map(lambda x: x.contiguous(), pipe.prepare(noise, pos))
    _, _, nvec, ntxt, _ = pipe.prepare(noise, neg)
    den = lambda x, t, **k: pipe.model.denoise(x, img_ids, txt, txt_ids, vec, t, guidance=3.5, **k)
    nk = dict(neg_txt=ntxt, neg_y=nvec, cfg_scale=SCALE)
    assert torch.equal(full, pipe.unpack(den(img, ts, **nk).float(), 96, 64))
    assert torch.equal(pipe.generate(pos, guidance_mode="cfg", guidance_rescale=0.0, zero_init_steps=0, **gkw, **kw), full)
    # every mode == Flux.denoise with the dict
    for skw, sh in ((dict(guidance_rescale=0.7), dict(rescale=0.7)),
                    (dict(guidance_mode="apg", apg_eta=0.25, apg_norm_threshold=40.0, apg_momentum=-0.5),
                     dict(mode="apg", eta=0.25, norm_threshold=40.0, momentum=-0.5)),
                    (dict(guidance_mode="cfg_zero_star", zero_init_steps=2), dict(mode="cfg_zero_star", zero_init_steps=2))):
        a = pipe.generate(pos, **gkw, **skw, **kw)
        assert torch.isfinite(a).all() and not torch.equal(a, full)
        assert torch.equal(a, pipe.unpack(den(img, ts, guidance_shaping=sh, **nk).float(), 96, 64)), skw
    # true_cfg_interval with zero-init: evaluations are counted across slices.  Steps 0, 1 plain, 2 .. 5 guided, 6, 7 plain; zero_init_steps = 3
    # zeroes the prediction of evaluation 2 alone, the guided slice's first (its offset is 2)
    mid = pipe.generate(pos, true_cfg_interval=(0.25, 0.75), guidance_mode="cfg_zero_star", zero_init_steps=3, **gkw, **kw)
    x = den(img, ts[0:3])
    x = den(x, ts[2:7], guidance_shaping=dict(mode="cfg_zero_star", zero_init_steps=3, step_offset=2), **nk)
    x = den(x, ts[6:9])
    assert torch.equal(mid, pipe.unpack(x.float(), 96, 64))
    x = den(img, ts[0:3])
    y = den(x, ts[2:4], guidance_shaping=dict(mode="cfg_zero_star", zero_init_steps=3, step_offset=2), **nk)
    assert torch.equal(x, y), "the zero-initialised evaluation moved the latent"
    # heun: two evaluations per step but the last; zero_init_steps counts evaluations
    h = pipe.generate(pos, sampler="heun", guidance_mode="apg", apg_momentum=-0.5, zero_init_steps=1, **gkw, **kw)
    assert torch.isfinite(h).all()
