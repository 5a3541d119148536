"""Stochastic samplers on the GPU.  The fresh noise of euler_ancestral / dpmpp_2m_sde is generated INSIDE the update kernel
(csrc/update_step.hip: Philox4x32-10 + Box-Muller, solver_step_kernel's NOISE form) as a pure function of (ids of the image, evaluation index,
element).  The words are compared bit for bit with the numpy reference of tests/stochastic_util.py, the normals with float64 Box-Muller of
the same words, and kernel and engine bit for bit with the interpreter fed the normals fluxmi_philox_normal returns.  Model helpers are those
of tests/test_cfg_gpu.py, tests/test_inpaint_gpu.py and tests/test_solvers_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import flux_oracle as fo
import inpaint_util as iu
import solver_util as su
import stochastic_util as st
from test_cfg_gpu import IN_CHANNELS, LAYOUTS, QUANTS, SCALE, build, cond_kw, dup, inputs, prompts, rel_l2, tiny_config, tiny_pipeline, to_dev
from test_inpaint_gpu import has_buffer, kernel_masks, ws_bytes
from test_solvers_gpu import bits

pytestmark = pytest.mark.gpu

EVALS = (0, 1, 2 ** 31 - 1)
IDS3 = [(0xa4093822, 0x299f31d0, 0, 0), (0xa4093822, 0x299f31d0, 1, 0), (0x00000007, 0xffffffff, 2, 0x03707344)]
SIZES = (960, 262144)  # 15 odd rows x 64; B x 262144 / 8 vectors: more than 2^16 of them


def ids_tensor(ids, dev):
    return torch.tensor([[w if w < 2 ** 31 else w - 2 ** 32 for w in row] for row in ids], dtype=torch.int32, device=dev).contiguous()


def philox(dev, ids, n, ev, raw):
    """fluxmi_philox_normal -> [B, n] int32 words (raw) or fp32 normals"""
    from fluxmi import _lib, ops

    out = torch.full((len(ids), n), -1 if raw else float("nan"), dtype=torch.int32 if raw else torch.float32, device=dev)
    d_ids = ids_tensor(ids, dev)
    _lib.call("fluxmi_philox_normal", ops._p(out), ops._p(d_ids), len(ids), n, ev, int(raw), ops._stream())
    torch.cuda.synchronize()
    return out


_REF = {}


def ref_words(n):
    """numpy's words for IDS3 at EVALS, computed once: {eval: uint32 [3, n]}"""
    if n not in _REF:
        _REF[n] = {ev: np.stack([st.words(ids, n, ev) for ids in IDS3]) for ev in EVALS}
    return _REF[n]


# ---- 1. the generator's words ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_philox_words_equal_numpy(dev, n):
    for ev in EVALS:
        got = philox(dev, IDS3, n, ev, raw=True).cpu().numpy().view(np.uint32)
        want = ref_words(n)[ev]
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"n={n} eval={ev}: {len(bad)} words differ, first at {bad[0]}: {got[tuple(bad[0])]:08x} vs {want[tuple(bad[0])]:08x}"


def test_philox_normal_refusals(dev):
    from fluxmi import _lib, ops

    out = torch.zeros(2, 64, dtype=torch.float32, device=dev)
    d_ids = ids_tensor(IDS3[:2], dev)
    for b, n, raw in ((2, 60, 0), (2, 4, 0), (-1, 64, 0), (2, -8, 0), (2, 64, 2)):
        with pytest.raises(RuntimeError, match="philox_normal: bad shape"):
            _lib.call("fluxmi_philox_normal", ops._p(out), ops._p(d_ids), b, n, 0, raw, ops._stream())
    with pytest.raises(RuntimeError, match="philox_normal: NULL argument"):
        _lib.call("fluxmi_philox_normal", None, ops._p(d_ids), 2, 64, 0, 0, ops._stream())
    with pytest.raises(RuntimeError, match="philox_normal: NULL argument"):
        _lib.call("fluxmi_philox_normal", ops._p(out), None, 2, 64, 0, 0, ops._stream())
    _lib.call("fluxmi_philox_normal", ops._p(out), ops._p(d_ids), 0, 64, 0, 0, ops._stream())  # an empty batch is no error
    torch.cuda.synchronize()
    assert not out.any()


# ---- 2. the normals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_philox_normals_against_float64(dev, n):
    """|z - z64| <= 16 * 2^-24 * max(1, |z64|): logf, sqrtf and sincospif are documented at about 1 ulp each and their arguments are exact
    by construction, so the chain stays under 5 ulp; the gate allows 3 x that."""
    worst = 0.0
    for ev in EVALS:
        z = philox(dev, IDS3, n, ev, raw=False).cpu().numpy().astype(np.float64)
        assert np.isfinite(z).all()
        for b in range(3):
            z64 = st.normals64(ref_words(n)[ev][b])
            ratio = np.abs(z[b] - z64) / (2.0 ** -24 * np.maximum(1.0, np.abs(z64)))
            worst = max(worst, ratio.max())
            print(f"n={n} eval={ev} image {b}: worst error {ratio.max():.2f} x 2^-24 max(1, |z|), mean {z[b].mean():+.4f} var {z[b].var():.4f}")
            assert ratio.max() <= 16.0, f"n={n} eval={ev} image {b}: {ratio.max():.2f} x 2^-24 at element {ratio.argmax()}"
    print(f"n={n}: worst {worst:.2f}")


# ---- 3. the kernel against the interpreter ------------------------------------------------------------------------------------------------
def kernel_rows():
    from fluxmi import solvers

    anc = solvers.build_program("euler_ancestral", [0.85, 0.6, 0.3])
    sde = solvers.build_program("dpmpp_2m_sde", [0.9, 0.65, 0.4, 0.2], eta=0.5)
    assert anc.coef[1][7] != 0.0 and sde.coef[1][3] != 0.0 and sde.coef[1][7] != 0.0 and sde.ctl[1][2] == 0
    return [
        ((0.75, 0.3, -0.0625, 0.41, -0.17, 0.9, -0.6, 0.37), (1, 1, 0, 1)),  # every term present, plus noise
        (anc.coef[1], anc.ctl[1]),                                            # an ancestral row
        (sde.coef[1], sde.ctl[1]),                                            # an SDE row: reads slot 0, writes slot 1
        ((0.75, 0.3, -0.0625, 0.41, -0.17, 0.9, -0.6, 0.0), (1, 1, 0, 1)),    # cn = 0: fluxmi_solver_step's result
    ]


TNEXT = [0.7313, 0.40625, 0.25, 0.0]
OFFSET = 5


@pytest.mark.parametrize("blend", ["off", "linear"])
@pytest.mark.parametrize("guided", [False, True], ids=["plain_update", "guided_update"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("B", [1, 3])
def test_solver_step_noise_kernel_bit_exact(dev, layout, B, guided, blend):
    from fluxmi import _lib, ops

    R, Rp, Ci, Co = LAYOUTS[layout]
    rows = kernel_rows()
    g = torch.Generator().manual_seed(177 + B)
    coef = torch.tensor([r[0] for r in rows], dtype=torch.float64).to(torch.float32).to(dev).contiguous()
    ctl = torch.tensor([r[1] for r in rows], dtype=torch.int32, device=dev).contiguous()
    d_tn = torch.tensor(TNEXT, dtype=torch.float32, device=dev)
    d_om = torch.tensor([1.0 - t for t in TNEXT], dtype=torch.float32, device=dev)
    d_scale = torch.tensor([SCALE], dtype=torch.float32, device=dev)
    d_off = torch.tensor([OFFSET], dtype=torch.int32, device=dev)
    ids = IDS3[:B]
    d_ids = ids_tensor(ids, dev)
    nb = 2 * B if guided else B
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(torch.bfloat16).to(dev)
    x0, noise = rnd(B, Rp, Co), rnd(B, Rp, Co)
    m = kernel_masks(B, Rp, Co, g)["soft"].to(dev)
    on = blend != "off"

    def call(img, pred, xs, hist, step_ptr, b=B, rows_=R, prows=Rp, ids_=d_ids, off=d_off, entry="fluxmi_solver_step_noise", lo=0):
        sl = lambda t: t[lo:lo + b] if t is not None else None
        args = [ops._p(img), ops._p(pred), ops._p(xs), ops._p(hist), ops._p(coef), ops._p(ctl), ops._p(sl(x0)) if on else None,
                ops._p(sl(noise)) if on else None, ops._p(sl(m)) if on else None, ops._p(d_tn), ops._p(d_om), None, step_ptr,
                ops._p(d_scale) if guided else None, b, rows_, prows, Ci, Co]
        if entry == "fluxmi_solver_step_noise":
            args += [ops._p(ids_) if ids_ is not None else None, ops._p(off) if off is not None else None]
        _lib.call(entry, *args, ops._stream())
        torch.cuda.synchronize()

    d_steps = [torch.tensor([j], dtype=torch.int32, device=dev) for j in range(len(rows))]  # alive until the kernels that read them are done
    for j, (row, c) in enumerate(rows):
        for off in ((d_off, OFFSET), (None, 0)) if j == 0 else ((d_off, OFFSET),):  # eval_offset = NULL reads as 0
            tag = f"{layout} B={B} row={j} guided={guided} blend={blend} offset={off[1]}"
            # guided: the two halves of the stream start DIFFERENT: the kernel reads x from the prompt half alone and writes both
            img, pred = rnd(nb, R, Ci), rnd(nb, Rp, Co)
            xs, hist = rnd(B, Rp, Co), torch.randn(2, B, Rp, Co, generator=g).to(dev)
            start = (img.clone(), xs.clone(), hist.clone())
            kept = [t.clone() for t in (pred, x0, noise, m, coef, ctl, d_ids, d_off)]
            z = philox(dev, ids, Rp * Co, j + off[1], raw=False).reshape(B, Rp, Co)
            w_xs, w_hist = xs.clone(), hist.clone()
            bl = (x0, noise, m, TNEXT[j], None) if on else None
            x = img[:B, :Rp, :Co].clone()
            want = st.apply_row(x, (pred[:B], pred[B:]) if guided else pred, row, c, w_xs, w_hist, z=z, scale=SCALE if guided else None, blend=bl)
            call(img, pred, xs, hist, ops._p(d_steps[j]), off=off[0])
            got = img[:B, :Rp, :Co]
            assert torch.isfinite(got).all() and torch.equal(got, want), f"{tag}: rel-L2 {rel_l2(got, want):.3e}"
            if guided:
                assert not torch.equal(start[0][:B], start[0][B:]) and torch.equal(img[B:, :Rp, :Co], got), f"{tag}: the halves differ after the update"
            assert torch.equal(img[:, Rp:], start[0][:, Rp:]), f"{tag}: reference rows changed"
            assert torch.equal(img[..., Co:], start[0][..., Co:]), f"{tag}: conditioning channels changed"
            assert all(torch.equal(a, b) for a, b in zip(kept, (pred, x0, noise, m, coef, ctl, d_ids, d_off))), f"{tag}: an input changed"
            assert torch.equal(bits(xs), bits(w_xs)) and torch.equal(bits(hist), bits(w_hist)), f"{tag}: xs / hist"
            if row[7] != 0.0:  # the noise is there: the deterministic kernel on the same inputs gives something else
                i2, x2, h2 = (t.clone() for t in start)
                call(i2, pred, x2, h2, ops._p(d_steps[j]), entry="fluxmi_solver_step")
                assert not torch.equal(i2[:B, :Rp, :Co], got), f"{tag}: the noise term changed nothing"
            else:  # cn == 0: fluxmi_solver_step's bits, xs and hist included
                i2, x2, h2 = (t.clone() for t in start)
                call(i2, pred, x2, h2, ops._p(d_steps[j]), entry="fluxmi_solver_step")
                assert torch.equal(i2, img) and torch.equal(bits(x2), bits(xs)) and torch.equal(bits(h2), bits(hist)), f"{tag}: cn = 0 differs"
            if B > 1 and j < 2:  # image b of the batch == the B = 1 launch with its ids alone
                for b in range(B):
                    pick = lambda t: torch.cat((t[b:b + 1], t[B + b:B + b + 1]), 0).contiguous() if guided else t[b:b + 1].contiguous()
                    i1, p1 = pick(start[0]), pick(pred)
                    x1, h1 = start[1][b:b + 1].contiguous(), start[2][:, b:b + 1].contiguous()
                    call(i1, p1, x1, h1, ops._p(d_steps[j]), b=1, ids_=d_ids[b:b + 1].contiguous(), off=off[0], lo=b)
                    assert torch.equal(i1[0], img[b]), f"{tag}: image {b} depends on its batch"
    # NULL ids and malformed shapes are refused with a message, and nothing is written
    img, pred, xs, hist = rnd(nb, R, Ci), rnd(nb, Rp, Co), rnd(B, Rp, Co), torch.zeros(2, B, Rp, Co, device=dev)
    before = [t.clone() for t in (img, xs, hist)]
    with pytest.raises(RuntimeError, match="solver_step_noise: NULL ids"):
        call(img, pred, xs, hist, ops._p(d_steps[0]), ids_=None)
    with pytest.raises(RuntimeError, match="solver_step: bad shape"):
        call(img, pred, xs, hist, None, rows_=Rp, prows=R + 1)
    with pytest.raises(RuntimeError, match="solver_step: bad shape"):
        call(img, pred, xs, hist, None, b=-1)
    with pytest.raises(RuntimeError, match="solver_step: NULL argument"):
        _lib.call("fluxmi_solver_step_noise", ops._p(img), ops._p(pred), None, ops._p(hist), ops._p(coef), ops._p(ctl), None, None, None, None, None,
                  None, None, None, B, R, Rp, Ci, Co, ops._p(d_ids), None, ops._stream())
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (img, xs, hist)))


# ---- the request of the model-level tests -----------------------------------------------------------------------------------------------
STOCHASTIC = ("euler_ancestral", "dpmpp_2m_sde")
ETA = {"euler_ancestral": 1.0, "dpmpp_2m_sde": 0.5}


def program(name, ts):
    from fluxmi import solvers

    return solvers.build_program(name, ts, ETA[name]) if name in STOCHASTIC else solvers.build_program(name, ts)


def denoise(model, d, ts, name=None, ids=None, off=0, img=None, inp=None, guided=False, **kw):
    if name is not None:
        kw["solver"] = program(name, ts)
    if ids is not None:
        kw["solver_noise"] = (ids, off)
    if guided:
        kw.update(neg_txt=d["neg_txt"], neg_y=d["neg_y"], cfg_scale=SCALE)
    if inp is not None:
        kw.update(inpaint_x0=inp[0], inpaint_noise=inp[1], inpaint_mask=inp[2])
    return model.denoise(d["img"] if img is None else img, d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts, guidance=3.5, **cond_kw(d), **kw)


def host_loop(model, d, ts, name, ids, x, mode, off=0, inp=None, guided=False):
    """model(...) per evaluation of the program and the interpreter's update on the normals fluxmi_philox_normal gives (ids, j + off);
    mode None = the model's own (calibrating, then frozen)"""
    prog = program(name, ts)
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
        z = philox(x.device, ids, x.shape[1] * x.shape[2], j + off, raw=False).reshape(x.shape) if row[7] != 0.0 else None
        bl = (inp[0], inp[1], inp[2], prog.times[j + 1], None) if inp is not None else None
        x = st.apply_row(x, (pred[:B], pred[B:]) if guided else pred, row, c, xs, hist, z=z, scale=SCALE if guided else None, blend=bl)
    return x


def ids_for(seed, B):
    return [st.ids_of(seed, k) for k in range(B)]


# ---- 4. stochastic denoise: graph == eager == host loop, through calibration and frozen ------------------------------------------------------
@pytest.mark.parametrize("name", STOCHASTIC)
@pytest.mark.parametrize("kind", list(IN_CHANNELS))
@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_stochastic_denoise_bit_exact(dev, qname, kind, name):
    cfg = tiny_config(kind)
    model, _ = build(cfg, QUANTS[qname], dev)
    ref, _ = build(cfg, QUANTS[qname], dev)  # the same weights: the host loop's own model, calibrated by its own forwards
    d = to_dev(inputs(kind, cfg.params, 64, 64, 32, 2, seed=5), dev)
    kept = {k: d[k].clone() for k in ("seq", "cond", "img") if k in d}
    ts = fo.get_schedule(16, d["img"].shape[1])
    ids = ids_for((3 << 32) + 12345, 2)
    # a fresh model's first request: the whole schedule's 16 evaluations: fp8 runs 13 calibrating evaluations (the noise kernel behind each),
    # one eager frozen one, then replays
    lat = denoise(model, d, ts, name, ids)
    assert lat.shape == d["img"].shape and lat.dtype == torch.bfloat16 and torch.isfinite(lat).all()
    want = host_loop(ref, d, ts, name, ids, d["img"].clone(), None)
    assert torch.equal(lat, want), f"through calibration: engine vs host loop rel-L2 {rel_l2(lat, want):.3e}"
    if qname == "fp8":
        assert model.calibration_state()[0] and ref.calibration_state()[0]
    mode = 1 if qname == "fp8" else 2
    ts2 = ts[8:]
    assert ts2[-1] == 0.0
    outs = {}
    for nm in STOCHASTIC:
        a = denoise(model, d, ts2, nm, ids, off=3, img=lat)
        b = denoise(model, d, ts2, nm, ids, off=3, img=lat, use_graph=False)
        assert torch.equal(a, b), f"{nm}: graph vs eager rel-L2 {rel_l2(a, b):.3e}"
        c = host_loop(model, d, ts2, nm, ids, lat.clone(), mode, off=3)
        assert torch.equal(a, c), f"{nm}: graph loop vs host loop rel-L2 {rel_l2(a, c):.3e}"
        assert torch.isfinite(a).all()
        outs[nm] = a
    assert not torch.equal(outs["euler_ancestral"], outs["dpmpp_2m_sde"])
    for k, v in kept.items():
        assert torch.equal(d[k], v), f"the caller's {k} changed"


def test_stochastic_composes_with_guidance_and_the_blend(dev):
    cfg = tiny_config()
    model, _ = build(cfg, QUANTS["fp8"], dev)
    d = to_dev(inputs("plain", cfg.params, 64, 64, 32, 2, seed=5), dev)
    inp = iu.make_inpaint(2, d["img"].shape[1], 64, 5, device=dev)
    ts = fo.get_schedule(16, d["img"].shape[1])
    ids = ids_for(99, 2)
    lat = denoise(model, d, ts[:14], "euler_ancestral", ids, use_graph=False)
    assert model.calibration_state()[0]
    ts2 = ts[8:]
    for name in STOCHASTIC:
        kw = dict(guided=True, inp=inp)
        a = denoise(model, d, ts2, name, ids, img=lat, **kw)
        b = denoise(model, d, ts2, name, ids, img=lat, use_graph=False, **kw)
        c = host_loop(model, d, ts2, name, ids, lat.clone(), 1, **kw)
        assert torch.equal(a, b) and torch.equal(a, c), f"{name}: graph vs eager {rel_l2(a, b):.3e}, vs host loop {rel_l2(a, c):.3e}"
        assert not torch.equal(a, denoise(model, d, ts2, name, ids, img=lat))
        me = inp[2].expand_as(a)  # the schedule ends at 0: every kept element is the init latent, bit for bit
        assert torch.equal(a[me == 0], inp[0][me == 0])


# ---- 5. graphs, seeds and cuts -------------------------------------------------------------------------------------------------------------
def test_one_graph_serves_every_seed_and_offset(dev):
    from fluxmi import _lib, ops, solvers

    cfg = tiny_config()
    model, _ = build(cfg, QUANTS["fp8"], dev)
    d = to_dev(inputs("plain", cfg.params, 64, 64, 32, 2, seed=5), dev)
    ts = fo.get_schedule(16, d["img"].shape[1])
    lat = denoise(model, d, ts[:14], use_graph=False)  # a PLAIN calibration
    ts2 = ts[8:]
    N = len(ts2) - 1
    plain, heun = denoise(model, d, ts2, img=lat), denoise(model, d, ts2, "heun", img=lat)
    assert has_buffer(model, "sol_xs") and not has_buffer(model, "sol_ids"), "a request without noise allocated the noise ids"
    ws = ws_bytes(model)
    s1, s2 = ids_for(11, 2), ids_for(12, 2)
    runs = [lambda: denoise(model, d, ts2, "euler_ancestral", s1, img=lat), lambda: denoise(model, d, ts2, "euler_ancestral", s2, img=lat),
            lambda: denoise(model, d, ts2, img=lat), lambda: denoise(model, d, ts2, "heun", img=lat),
            lambda: denoise(model, d, ts2, "euler_ancestral", s1, img=lat), lambda: denoise(model, d, ts2, "dpmpp_2m_sde", s1, img=lat)]
    got = [r() for r in runs]
    assert has_buffer(model, "sol_ids") and ws_bytes(model) == ws + (2 * 16 + 4 + 255) // 256 * 256
    assert torch.equal(got[0], got[4]), "the same seed twice gives different bits"
    assert not torch.equal(got[0], got[1]), "two seeds give the same bits"
    assert torch.equal(got[2], plain) and torch.equal(got[3], heun), "a request behind a noise request differs from its earlier result"
    assert not torch.equal(got[0], plain) and not torch.equal(got[5], got[0])
    # a cut request: N evaluations in one call == k, then N - k with eval_offset = k (euler_ancestral carries no history over the cut)
    for k in (1, 3):
        head = denoise(model, d, ts2[:k + 1], "euler_ancestral", s1, img=lat)
        tail = denoise(model, d, ts2[k:], "euler_ancestral", s1, off=k, img=head)
        assert torch.equal(tail, got[0]), f"cut at {k}: rel-L2 {rel_l2(tail, got[0]):.3e}"
        assert not torch.equal(denoise(model, d, ts2[k:], "euler_ancestral", s1, off=0, img=head), got[0]), "the offset does nothing"
    # the engine's refusals; the next calls are untouched by the leftovers
    prog, det = program("euler_ancestral", ts2), solvers.build_program("heun", ts2)
    tab = lambda p: ((C.c_double * (8 * len(p.coef)))(*[v for r in p.coef for v in r]), (C.c_int * (4 * len(p.ctl)))(*[v for r in p.ctl for v in r]),
                     len(p.coef))
    flat = lambda ids: (C.c_uint32 * (4 * len(ids)))(*[w for r in ids for w in r])
    t_io, tsc = C.c_int(0), (C.c_double * len(ts2))(*ts2)
    img = lat.clone()
    run = lambda: _lib.call("fluxmi_engine_denoise", model._engine, ops._p(img), ops._p(d["txt"]), ops._p(d["y"]), 3.5, tsc, N, C.byref(t_io), 1,
                            ops._stream())
    with model._lock:
        _lib.call("fluxmi_engine_set_solver", model._engine, *tab(prog))
        with pytest.raises(RuntimeError, match="no ids are set"):
            run()
        _lib.call("fluxmi_engine_set_solver_noise", model._engine, flat(s1[:1]), 1, 0)
        with pytest.raises(RuntimeError, match="ids of 1 images"):
            run()
        for ids, b, off, msg in ((s1, 0, 0, "batch"), (s1 + s1, 3, 0, "batch"), (s1, 2, -1, "eval_offset"), (None, 2, 0, "NULL")):
            with pytest.raises(RuntimeError, match=msg):
                _lib.call("fluxmi_engine_set_solver_noise", model._engine, flat(ids) if ids else None, b, off)
        _lib.call("fluxmi_engine_set_solver", model._engine, *tab(det))
        with pytest.raises(RuntimeError, match="no non-zero noise coefficient"):
            _lib.call("fluxmi_engine_set_solver_noise", model._engine, flat(s1), 2, 0)
        _lib.call("fluxmi_engine_set_solver", model._engine, None, None, 0)
        with pytest.raises(RuntimeError, match="fluxmi_engine_set_solver first"):
            _lib.call("fluxmi_engine_set_solver_noise", model._engine, flat(s1), 2, 0)
    torch.cuda.synchronize()
    assert torch.equal(img, lat)
    assert torch.equal(runs[2](), plain) and torch.equal(runs[0](), got[0])
    # each result equals a fresh engine's
    for i in (0, 1, 5):
        model._invalidate_engine()
        fresh = runs[i]()
        assert torch.equal(got[i], fresh), f"request {i} on the shared engine differs from a fresh engine: rel-L2 {rel_l2(got[i], fresh):.3e}"
    model._invalidate_engine()
    assert torch.equal(runs[2](), plain) and not has_buffer(model, "sol_ids") and not has_buffer(model, "sol_xs")


# ---- 6. batch invariance ---------------------------------------------------------------------------------------------------------------
def test_a_stochastic_sample_does_not_depend_on_its_batch(dev):
    cfg = tiny_config()
    model, _ = build(cfg, QUANTS["fp8"], dev)
    d = to_dev(inputs("plain", cfg.params, 64, 64, 32, 3, seed=9), dev)
    ts = fo.get_schedule(16, d["img"].shape[1])
    lat = denoise(model, d, ts[:14], use_graph=False)
    ts2 = ts[8:]
    ids = ids_for(2024, 3)
    for name in STOCHASTIC:
        all3 = denoise(model, d, ts2, name, ids, img=lat)
        assert not torch.equal(all3[0], all3[1])
        for b in range(3):
            one = denoise(model, {k: v[b:b + 1] for k, v in d.items()}, ts2, name, ids[b:b + 1], img=lat[b:b + 1])
            assert torch.equal(one[0], all3[b]), f"{name}: sample {b} depends on its batch: rel-L2 {rel_l2(one[0], all3[b]):.3e}"


# ---- 7. pipeline -----------------------------------------------------------------------------------------------------------------------
def test_pipeline_stochastic_samplers(dev):
    pipe = tiny_pipeline(dev)
    pipe.compile()
    pos, _ = prompts()
    kw = dict(width=64, height=96, num_steps=6, seed=7, silent=True, output_type="latent")
    plain = pipe.generate(pos, **kw)
    assert torch.equal(pipe.generate(pos, sampler="euler", **kw), plain), "sampler='euler' is not today's call"
    for req, det in ((dict(sampler="euler_ancestral"), plain), (dict(sampler="dpmpp_2m_sde", eta=0.5), pipe.generate(pos, sampler="dpmpp_2m", **kw))):
        a = pipe.generate(pos, **req, **kw)
        assert a.shape == plain.shape and torch.isfinite(a).all()
        assert torch.equal(pipe.generate(pos, **req, **kw), a), f"{req}: the same seed gives different latents"
        assert not torch.equal(pipe.generate(pos, noise_seed=8, **req, **kw), a), f"{req}: noise_seed changes nothing"
        assert torch.equal(pipe.generate(pos, noise_seed=7, **req, **kw), a), f"{req}: the default noise seed is not the request's seed"
        assert not torch.equal(a, det), f"{req}: equals its deterministic counterpart"
    # == model.denoise on prepare's tensors with the program and the ids of the request
    from fluxmi import solvers

    generator, seed = pipe.set_seed(7)
    noise, ts = pipe.preprocess_latent(height=96, width=64, num_steps=6, generator=generator, num_images=1)
    img, img_ids, vec, txt, txt_ids = map(lambda x: x.contiguous(), pipe.prepare(noise, pos))
    want = pipe.model.denoise(img, img_ids, txt, txt_ids, vec, ts, guidance=3.5, solver=solvers.build_program("euler_ancestral", ts),
                              solver_noise=([st.ids_of(seed, 0)], 0))
    assert torch.equal(pipe.generate(pos, sampler="euler_ancestral", **kw), pipe.unpack(want.float(), 96, 64))
    px = torch.as_tensor(pipe.generate(pos, sampler="euler_ancestral", **dict(kw, output_type="uint8")))
    assert px.dtype == torch.uint8 and tuple(px.shape) == (1, 96, 64, 3) and px.float().std() > 0
    # requests and slices that draw nothing run (no ids travel with them): eta = 0, s_noise = 0, one step, and a guided interval that
    # leaves only the deterministic step onto sigma 0 as the last slice (6 steps, guided on [0, 5))
    _, neg = prompts()
    for name in STOCHASTIC:
        for req in (dict(eta=0.0), dict(s_noise=0.0), dict(num_steps=1)):
            r = dict(kw, sampler=name, **req)
            a = pipe.generate(pos, **r)
            assert torch.isfinite(a).all() and torch.equal(pipe.generate(pos, noise_seed=8, **r), a), f"{name} {req}: noise where none is drawn"
        r = dict(kw, sampler=name, negative_prompt=neg, true_cfg_scale=2.0, true_cfg_interval=(0.0, 0.8))
        a = pipe.generate(pos, **r)
        assert torch.isfinite(a).all() and torch.equal(pipe.generate(pos, **r), a) and not torch.equal(pipe.generate(pos, noise_seed=8, **r), a)
    assert torch.equal(pipe.generate(pos, **kw), plain)
