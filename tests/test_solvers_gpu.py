"""Higher-order samplers on the GPU.  Every update of a solver request is ONE kernel (csrc/update_step.hip, solver_step_kernel) driven by
device tables: row j of the program (fluxmi/solvers.py) says how evaluation j combines x, the saved iterate, g = ga x + gb v and two fp32
history slots.  The kernel and the engine are compared bit for bit with the interpreter of tests/solver_util.py (exact=False: fp32 products
and sums rounded one by one, no fma, one bf16 store).  Model helpers are those of tests/test_cfg_gpu.py and tests/test_inpaint_gpu.py."""
import ctypes as C

import pytest
import torch

import flux_oracle as fo
import inpaint_util as iu
import solver_util as su
from test_cfg_gpu import IN_CHANNELS, KNOB_SETS, LAYOUTS, QUANTS, SCALE, build, cond_kw, dup, inputs, prompts, rel_l2, tiny_config, tiny_pipeline, to_dev
from test_inpaint_gpu import has_buffer, kernel_masks, ws_bytes

pytestmark = pytest.mark.gpu

NAN = float("nan")
# the rows of the kernel test: (coef, ctl, what is pre-filled with NaN because the row must not read it)
ROWS = [
    # every coefficient non-zero, the slot written is the slot read as h2, the iterate saved
    ((0.75, 0.3, -0.0625, 0.41, -0.17, 0.9, -0.6, 0.0), (1, 1, 0, 1), ()),
    # Euler: nothing saved, nothing kept, xs and both slots unread
    ((1.0, 0.0, -0.03173828125, 0.0, 0.0, 0.0, 1.0, 0.0), (0, -1, -1, -1), ("xs", "h0", "h1")),
    # non-zero history coefficients whose slots are -1; g kept in slot 0; cx == 0
    ((0.0, 0.0, 1.0, 0.5, 0.25, 1.0, -0.7, 0.0), (0, 0, -1, -1), ("xs", "h0", "h1")),
    # zero coefficients with valid slots (c0, c1): g is not needed at all; slot 1 is read, the iterate saved over an unread xs
    ((0.5, 0.0, 0.0, 0.0, 0.3, 0.0, 0.0, 0.0), (1, -1, 0, 1), ("xs", "h0")),
]
TNEXT = [0.7313, 0.40625, 0.0, 0.25]
THR = [0.3, 0.75, 0.5, 0.3]


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def tables(dev, rows=ROWS):
    coef = torch.tensor([r[0] for r in rows], dtype=torch.float64).to(torch.float32).to(dev).contiguous()
    ctl = torch.tensor([r[1] for r in rows], dtype=torch.int32, device=dev).contiguous()
    return coef, ctl


# ---- 1. the kernel against the interpreter ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend", ["off", "linear", "differential"])
@pytest.mark.parametrize("guided", [False, True], ids=["plain_update", "guided_update"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("B", [1, 3])
def test_solver_step_kernel_bit_exact(dev, layout, B, guided, blend):
    from fluxmi import _lib, ops

    R, Rp, Ci, Co = LAYOUTS[layout]
    g = torch.Generator().manual_seed(77 + B)
    coef, ctl = tables(dev)
    d_tn = torch.tensor(TNEXT, dtype=torch.float32, device=dev)
    d_om = torch.tensor([1.0 - t for t in TNEXT], dtype=torch.float32, device=dev)
    d_thr = torch.tensor(THR, dtype=torch.float32, device=dev)
    d_scale = torch.tensor([SCALE], dtype=torch.float32, device=dev)
    nb = 2 * B if guided else B
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(torch.bfloat16).to(dev)
    x0, noise = rnd(B, Rp, Co), rnd(B, Rp, Co)
    m = kernel_masks(B, Rp, Co, g)["soft"].to(dev)

    def call(img, pred, xs, hist, step_ptr, b=B, rows=R, prows=Rp, x0_=x0, coef_=coef):
        on = blend != "off"
        _lib.call("fluxmi_solver_step", ops._p(img), ops._p(pred), ops._p(xs), ops._p(hist), ops._p(coef_) if coef_ is not None else None,
                  ops._p(ctl), ops._p(x0_) if on and x0_ is not None else None, ops._p(noise) if on else None, ops._p(m) if on else None,
                  ops._p(d_tn), ops._p(d_om), ops._p(d_thr) if blend == "differential" else None, step_ptr,
                  ops._p(d_scale) if guided else None, b, rows, prows, Ci, Co, ops._stream())
        torch.cuda.synchronize()

    def case(j, step_ptr):
        row, c, nan = ROWS[j]
        # guided: the two halves of the stream start DIFFERENT: the kernel must read x from the prompt half alone and write both
        img, pred = rnd(nb, R, Ci), rnd(nb, Rp, Co)
        xs = torch.full((B, Rp, Co), NAN, dtype=torch.bfloat16, device=dev) if "xs" in nan else rnd(B, Rp, Co)
        hist = torch.randn(2, B, Rp, Co, generator=g).to(dev)
        for s in (0, 1):
            if f"h{s}" in nan:
                hist[s] = NAN
        before, kept = img.clone(), [t.clone() for t in (pred, x0, noise, m, coef, ctl)]
        x = img[:B, :Rp, :Co].clone()
        w_xs, w_hist = xs.clone(), hist.clone()
        bl = None if blend == "off" else (x0, noise, m, TNEXT[j], THR[j] if blend == "differential" else None)
        want = su.apply_row(x, (pred[:B], pred[B:]) if guided else pred, row, c, w_xs, w_hist, scale=SCALE if guided else None, blend=bl)
        assert want.dtype == torch.bfloat16 and torch.isfinite(want).all()
        call(img, pred, xs, hist, step_ptr)
        tag = f"{layout} B={B} row={j} guided={guided} blend={blend}"
        got = img[:B, :Rp, :Co]
        assert torch.isfinite(got).all(), f"{tag}: the kernel read a buffer its row skips"
        assert torch.equal(got, want), f"{tag}: rel-L2 {rel_l2(got, want):.3e}"
        if guided:
            assert torch.equal(img[B:, :Rp, :Co], got), f"{tag}: the halves differ after the update"
        assert torch.equal(img[:, Rp:], before[:, Rp:]), f"{tag}: reference rows changed"
        assert torch.equal(img[..., Co:], before[..., Co:]), f"{tag}: conditioning channels changed"
        assert all(torch.equal(a, b) for a, b in zip(kept, (pred, x0, noise, m, coef, ctl))), f"{tag}: an input changed"
        # xs / hist: the saved PRE-update iterate and g where the row says so, untouched (NaN payload included) everywhere else
        assert torch.equal(bits(xs), bits(w_xs)), f"{tag}: xs"
        assert torch.equal(bits(hist), bits(w_hist)), f"{tag}: hist"
        if c[0]:
            assert torch.equal(xs, x)
        else:
            assert torch.isnan(xs).all() == ("xs" in nan)

    d_steps = [torch.tensor([j], dtype=torch.int32, device=dev) for j in range(len(ROWS))]  # alive until the kernels that read them are done
    for j in range(len(ROWS)):
        case(j, ops._p(d_steps[j]))
    case(0, None)  # step = NULL reads row 0 of every table
    # malformed shapes and NULL arguments are refused with a message, and nothing is written
    img, pred, xs, hist = rnd(nb, R, Ci), rnd(nb, Rp, Co), rnd(B, Rp, Co), torch.zeros(2, B, Rp, Co, device=dev)
    before = [t.clone() for t in (img, xs, hist)]
    with pytest.raises(RuntimeError, match="solver_step: bad shape"):
        call(img, pred, xs, hist, None, rows=Rp, prows=R + 1)
    with pytest.raises(RuntimeError, match="solver_step: bad shape"):
        call(img, pred, xs, hist, None, b=-1)
    with pytest.raises(RuntimeError, match="solver_step: NULL argument"):
        call(img, pred, xs, hist, None, coef_=None)
    with pytest.raises(RuntimeError, match="solver_step: NULL argument"):
        _lib.call("fluxmi_solver_step", ops._p(img), ops._p(pred), None, ops._p(hist), ops._p(coef), ops._p(ctl), None, None, None, None, None, None,
                  None, None, B, R, Rp, Ci, Co, ops._stream())
    with pytest.raises(RuntimeError, match="solver_step: NULL argument"):  # the blend operands go together
        _lib.call("fluxmi_solver_step", ops._p(img), ops._p(pred), ops._p(xs), ops._p(hist), ops._p(coef), ops._p(ctl), ops._p(x0), None, ops._p(m),
                  ops._p(d_tn), ops._p(d_om), None, None, None, B, R, Rp, Ci, Co, ops._stream())
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (img, xs, hist)))


def test_solver_step_kernel_shape_refusals(dev):
    """both shorter and narrower, widths that are no multiple of 8"""
    from fluxmi import _lib, ops

    t = torch.zeros(2, 16, 64, dtype=torch.bfloat16, device=dev)
    h = torch.zeros(2, 2, 16, 64, dtype=torch.float32, device=dev)
    coef, ctl = tables(dev)
    for rows, prows, ci, co in ((16, 8, 64, 32), (16, 16, 64, 12), (16, 16, 60, 60), (16, 16, 32, 64)):
        with pytest.raises(RuntimeError, match="solver_step: bad shape"):
            _lib.call("fluxmi_solver_step", ops._p(t), ops._p(t), ops._p(t), ops._p(h), ops._p(coef), ops._p(ctl), None, None, None, None, None, None,
                      None, None, 1, rows, prows, ci, co, ops._stream())


# ---- the request of the model-level tests -----------------------------------------------------------------------------------------------
def denoise(model, d, ts, name=None, img=None, inp=None, thr=None, guided=False, **kw):
    from fluxmi import solvers

    if name is not None:
        kw["solver"] = solvers.build_program(name, ts)
    if guided:
        kw.update(neg_txt=d["neg_txt"], neg_y=d["neg_y"], cfg_scale=SCALE)
    if inp is not None:
        kw.update(inpaint_x0=inp[0], inpaint_noise=inp[1], inpaint_mask=inp[2], inpaint_thresholds=thr)
    return model.denoise(d["img"] if img is None else img, d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts, guidance=3.5, **cond_kw(d), **kw)


def host_loop(model, d, ts, name, x, mode, inp=None, thr=None, guided=False):
    """model(...) per EVALUATION of the program and the interpreter's update; mode None = the model's own (calibrating, then frozen)"""
    from fluxmi import solvers

    prog = solvers.build_program(name, ts)
    x = x.to(torch.bfloat16)
    B = x.shape[0]
    n = 2 * B if guided else B
    two = dup if guided else (lambda t: t)
    g = torch.full((n,), 3.5, dtype=torch.bfloat16, device=x.device)
    kw = {k: two(v) for k, v in cond_kw(d).items()}
    txt, y = (torch.cat((d["txt"], d["neg_txt"]), 0), torch.cat((d["y"], d["neg_y"]), 0)) if guided else (d["txt"], d["y"])
    xs, hist = su.new_state(x)
    for j, (row, c) in enumerate(zip(prog.coef, prog.ctl)):
        tv = torch.full((n,), prog.times[j], dtype=torch.bfloat16, device=x.device)
        pred = model(two(x), two(d["img_ids"]), txt, two(d["txt_ids"]), tv, y, g, mode=mode, **kw)
        bl = None
        if inp is not None:
            bl = (inp[0], inp[1], inp[2], prog.times[j + 1], None if thr is None else thr[prog.step_of_eval[j]])
        x = su.apply_row(x, (pred[:B], pred[B:]) if guided else pred, row, c, xs, hist, scale=SCALE if guided else None, blend=bl)
    return x


SAMPLERS = ("euler", "heun", "midpoint", "ab2", "dpmpp_2m")


# ---- 2. solver denoise: graph == eager == host loop, through calibration and frozen -----------------------------------------------------------
@pytest.mark.parametrize("cal", ["heun", "dpmpp_2m"])
@pytest.mark.parametrize("kind", list(IN_CHANNELS))
@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_solver_denoise_bit_exact(dev, qname, kind, cal):
    from fluxmi import _lib

    cfg = tiny_config(kind)
    model, _ = build(cfg, QUANTS[qname], dev)
    ref, _ = build(cfg, QUANTS[qname], dev)  # the same weights: the host loop's own model, calibrated by its own forwards
    d = to_dev(inputs(kind, cfg.params, 64, 64, 32, 2, seed=5), dev)
    kept = {k: d[k].clone() for k in ("seq", "cond", "img") if k in d}
    ts = fo.get_schedule(16, d["img"].shape[1])
    # a fresh model's first request, under a two-stage and under a multistep program: 11 Heun steps = 21 evaluations, or the whole schedule's
    # 16 dpmpp_2m evaluations: fp8 runs 13 calibrating evaluations (the solver kernel behind each), one eager frozen one, then replays
    ts1 = ts[:12] if cal == "heun" else ts
    lat = denoise(model, d, ts1, cal)
    assert lat.shape == d["img"].shape and lat.dtype == torch.bfloat16 and torch.isfinite(lat).all()
    want = host_loop(ref, d, ts1, cal, d["img"].clone(), None)
    assert torch.equal(lat, want), f"through calibration: engine vs host loop rel-L2 {rel_l2(lat, want):.3e}"
    if qname == "fp8":
        assert model.calibration_state()[0] and ref.calibration_state()[0]
    mode = 1 if qname == "fp8" else 2
    ts2 = ts[8:]
    assert ts2[-1] == 0.0
    outs = {}
    for name in SAMPLERS:
        a = denoise(model, d, ts2, name, img=lat)
        b = denoise(model, d, ts2, name, img=lat, use_graph=False)
        assert torch.equal(a, b), f"{name}: graph vs eager rel-L2 {rel_l2(a, b):.3e}"
        c = host_loop(model, d, ts2, name, lat.clone(), mode)
        assert torch.equal(a, c), f"{name}: graph loop vs host loop rel-L2 {rel_l2(a, c):.3e}"
        assert torch.isfinite(a).all()
        outs[name] = a
    assert len({bits(o).cpu().numpy().tobytes() for o in outs.values()}) == len(SAMPLERS), "two samplers gave the same latents"
    for k, v in kept.items():
        assert torch.equal(d[k], v), f"the caller's {k} changed"
    if qname == "fp8" and kind == "plain" and cal == "heun":
        for knobs in KNOB_SETS:
            with _lib.tuning(**knobs):
                a3 = denoise(model, d, ts2, "heun", img=lat)
            assert torch.equal(outs["heun"], a3), f"heun latents change under tuning {knobs}: rel-L2 {rel_l2(a3, outs['heun']):.3e}"


@pytest.mark.parametrize("name", ["heun", "dpmpp_2m"])
def test_solver_composes_with_guidance_and_the_blend(dev, name):
    cfg = tiny_config()
    model, _ = build(cfg, QUANTS["fp8"], dev)
    d = to_dev(inputs("plain", cfg.params, 64, 64, 32, 2, seed=5), dev)
    inp = iu.make_inpaint(2, d["img"].shape[1], 64, 5, device=dev)
    ts = fo.get_schedule(16, d["img"].shape[1])
    lat = denoise(model, d, ts[:12], "heun", use_graph=False)
    assert model.calibration_state()[0]
    ts2 = ts[8:]
    n = len(ts2) - 1
    thr = [1.0 - (i + 1) / n for i in range(n)]  # one per USER step
    plain = denoise(model, d, ts2, name, img=lat)
    for tag, kw in (("guided", dict(guided=True)), ("masked", dict(inp=inp)), ("differential", dict(inp=inp, thr=thr)),
                    ("guided + masked", dict(guided=True, inp=inp))):
        a = denoise(model, d, ts2, name, img=lat, **kw)
        b = denoise(model, d, ts2, name, img=lat, use_graph=False, **kw)
        c = host_loop(model, d, ts2, name, lat.clone(), 1, **kw)
        assert torch.equal(a, b) and torch.equal(a, c), f"{name} {tag}: graph vs eager {rel_l2(a, b):.3e}, vs host loop {rel_l2(a, c):.3e}"
        assert not torch.equal(a, plain), f"{name} {tag}: no effect"
        if "inp" in kw:  # the schedule ends at 0: every kept element is the init latent, bit for bit
            me = inp[2].expand_as(a)
            assert torch.equal(a[me == 0], inp[0][me == 0])


# ---- 3. the graph is keyed on the solver ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_plain_and_solver_requests_never_share_a_graph(dev, qname):
    from fluxmi import _lib, ops, solvers

    cfg = tiny_config()
    model, _ = build(cfg, QUANTS[qname], dev)
    d = to_dev(inputs("plain", cfg.params, 64, 64, 32, 2, seed=5), dev)
    ts = fo.get_schedule(16, d["img"].shape[1])
    lat = denoise(model, d, ts[:14], use_graph=False)  # a PLAIN calibration
    ts2 = ts[8:]
    first = denoise(model, d, ts2, img=lat)
    assert not has_buffer(model, "sol_xs") and not has_buffer(model, "sol_hist"), "a request without a solver allocated the solver buffers"
    ws = ws_bytes(model)
    runs = [lambda: denoise(model, d, ts2, img=lat), lambda: denoise(model, d, ts2, "heun", img=lat), lambda: denoise(model, d, ts2, img=lat),
            lambda: denoise(model, d, ts2, "ab2", img=lat), lambda: denoise(model, d, ts2, img=lat)]
    got = [r() for r in runs]
    elems = d["img"].numel()
    assert has_buffer(model, "sol_xs") and has_buffer(model, "sol_hist")
    assert ws_bytes(model) == ws + (elems * 2 + 255) // 256 * 256 + (2 * elems * 4 + 255) // 256 * 256
    assert all(torch.equal(got[i], first) for i in (0, 2, 4)), "a plain request behind a solver request differs from its earlier result"
    assert not torch.equal(got[1], first) and not torch.equal(got[3], first) and not torch.equal(got[1], got[3])
    # the saved iterate is readable: Heun's last two-stage step saved the iterate its last step started from ... (just its shape here)
    xs = torch.empty_like(d["img"])
    with model._lock:
        _lib.call("fluxmi_engine_copy_buffer", model._engine, b"sol_xs", 0, ops._p(xs), xs.numel() * 2, 0, ops._stream())
    torch.cuda.synchronize()
    assert torch.isfinite(xs).all()
    # a denoise call of another length than the program is refused; the next plain call is untouched by the leftover
    prog = solvers.build_program("heun", ts2)
    t_io, tsc = C.c_int(0), (C.c_double * len(ts2))(*ts2)
    coef = (C.c_double * (8 * len(prog.coef)))(*[v for r in prog.coef for v in r])
    ctl = (C.c_int * (4 * len(prog.ctl)))(*[v for r in prog.ctl for v in r])
    img = lat.clone()
    with model._lock:
        _lib.call("fluxmi_engine_set_solver", model._engine, coef, ctl, len(prog.coef))
        with pytest.raises(RuntimeError, match="solver program holds"):
            _lib.call("fluxmi_engine_denoise", model._engine, ops._p(img), ops._p(d["txt"]), ops._p(d["y"]), 3.5, tsc, len(ts2) - 1, C.byref(t_io), 1,
                      ops._stream())
        with pytest.raises(RuntimeError, match="out of range"):
            _lib.call("fluxmi_engine_set_solver", model._engine, coef, ctl, 1025)
        _lib.call("fluxmi_engine_set_solver", model._engine, None, None, 0)
    assert torch.equal(img, lat)
    assert torch.equal(denoise(model, d, ts2, img=lat), first)
    for i in (1, 3):
        model._invalidate_engine()
        fresh = runs[i]()
        assert torch.equal(got[i], fresh), f"request {i} on the shared engine differs from a fresh engine: rel-L2 {rel_l2(got[i], fresh):.3e}"
    model._invalidate_engine()
    assert torch.equal(runs[0](), first) and not has_buffer(model, "sol_xs")


# ---- 4. batch invariance ---------------------------------------------------------------------------------------------------------------
def test_a_heun_sample_does_not_depend_on_its_batch(dev):
    cfg = tiny_config()
    model, _ = build(cfg, QUANTS["fp8"], dev)
    d = to_dev(inputs("plain", cfg.params, 64, 64, 32, 3, seed=9), dev)
    ts = fo.get_schedule(16, d["img"].shape[1])
    lat = denoise(model, d, ts[:14], use_graph=False)
    ts2 = ts[8:]
    both = denoise(model, d, ts2, "heun", img=lat)
    for b in range(3):
        one = denoise(model, {k: v[b:b + 1] for k, v in d.items()}, ts2, "heun", img=lat[b:b + 1])
        assert torch.equal(one[0], both[b]), f"sample {b} depends on its batch: rel-L2 {rel_l2(one[0], both[b]):.3e}"


# ---- 5. pipeline -----------------------------------------------------------------------------------------------------------------------
def test_pipeline_samplers(dev):
    pipe = tiny_pipeline(dev)
    pipe.compile()
    pos, _ = prompts()
    kw = dict(width=64, height=96, num_steps=6, seed=7, silent=True)
    plain = pipe.generate(pos, output_type="latent", **kw)
    assert torch.equal(pipe.generate(pos, sampler="euler", output_type="latent", **kw), plain), "sampler='euler' is not today's call"
    a = pipe.generate(pos, sampler="dpmpp_2m", sigma_schedule="karras", output_type="latent", **kw)
    b = pipe.generate(pos, sampler="heun", sigmas=[1.0, 0.85, 0.6, 0.3, 0.1], output_type="latent", **kw)
    for t in (a, b):
        assert t.shape == plain.shape and torch.isfinite(t).all() and not torch.equal(t, plain)
    px = torch.as_tensor(pipe.generate(pos, sampler="dpmpp_2m", sigma_schedule="karras", output_type="uint8", **kw))
    assert px.dtype == torch.uint8 and tuple(px.shape) == (1, 96, 64, 3) and px.float().std() > 0
    px = torch.as_tensor(pipe.generate(pos, sampler="heun", sigmas=[1.0, 0.85, 0.6, 0.3, 0.1], output_type="uint8", **kw))
    assert tuple(px.shape) == (1, 96, 64, 3)
    # == model.denoise on prepare's tensors with the program of the request's schedule
    from fluxmi import solvers

    generator, _ = pipe.set_seed(7)
    noise, ts = pipe.preprocess_latent(height=96, width=64, num_steps=6, generator=generator, num_images=1, sigma_schedule="karras")
    img, img_ids, vec, txt, txt_ids = map(lambda x: x.contiguous(), pipe.prepare(noise, pos))
    want = pipe.model.denoise(img, img_ids, txt, txt_ids, vec, ts, guidance=3.5, solver=solvers.build_program("dpmpp_2m", ts))
    assert torch.equal(a, pipe.unpack(want.float(), 96, 64))
    with pytest.raises(ValueError, match="cache_threshold"):
        pipe.generate(pos, sampler="heun", cache_threshold=0.1, **kw)
