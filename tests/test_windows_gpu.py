"""Tiled generation on the GPU (include/fluxmi.h: fluxmi_window_gather / _step, fluxmi_engine_set_windows / _denoise_windows; DESIGN.md
section 7).  The latent of a tiled request is one canvas [N, Hc, Wc, C] beside the image stream, which holds its S = N * ny * nx overlapping
windows as samples of one engine batch (2S guided).  Kernel and engine are checked bit for bit against tests/window_ref.py's restatement of
the header's formulas; the oracle loop is FluxOracle.forward on the window batch plus that restatement.  Model helpers are those of
tests/test_cfg_gpu.py (hidden 256, 2 + 2 blocks, Lt 32); windows are 64 x 64 px = 4 x 4 tokens."""
import ctypes as C

import pytest
import torch

import flux_oracle as fo
import window_ref as wr
from test_cfg_gpu import QUANTS, build, guided_denoise, inputs, make_oracle, plain_denoise, prompts, rel_l2, tiny_config, tiny_pipeline, to_dev
from test_flowedit_gpu import captures

pytestmark = pytest.mark.gpu

SCALE = 3.5
HC, WC, WH, WW = 6, 10, 4, 4  # a 96 x 160 px canvas, 64 x 64 px windows


def make_plan(stride=(2, 3), profile="cosine", Hc=HC, Wc=WC, h=WH, w=WW):
    from fluxmi import windows

    return windows.plan(Hc, Wc, h, w, stride[0], stride[1], profile)


def dev_tables(p, dev):
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    return i32(p.row0), i32(p.col0), p.Ny.to(dev).contiguous(), p.Nx.to(dev).contiguous()


def f32(v):
    return torch.tensor(v, dtype=torch.float32).item()


# ---- 1. the kernel against the torch restatement ---------------------------------------------------------------------------------------
DTS = [-0.1875 + 2.0 ** -12, 0.3, -0.0712890625]


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("stride", [(2, 3), (2, 4), (1, 1)], ids=["s2x3", "snapped2x4", "s1x1"])
def test_window_kernels_bit_exact(dev, N, stride):
    from fluxmi import ops

    g = torch.Generator().manual_seed(100 * N + 10 * stride[0] + stride[1])
    rnd = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16)
    # bf16 NaN patterns: exponent all ones, a random non-zero mantissa
    nan = lambda *s: torch.randint(1, 128, s, generator=g, dtype=torch.int16).bitwise_or(0x7f80).view(torch.bfloat16)
    dts = torch.tensor(DTS, dtype=torch.float32, device=dev)
    sc = torch.tensor([SCALE], dtype=torch.float32, device=dev)
    for Cc in (64, 16):
        for profile in ("cosine", "uniform"):
            p = make_plan(stride, profile)
            if stride == (1, 1):
                assert p.ny == 3 and p.nx == 7 and max(sum(c0 <= c < c0 + WW for c0 in p.col0) for c in range(WC)) > 2
            if stride == (2, 4):
                assert p.col0 == [0, 4, 6]  # the snapped, irregular overlap
            row0, col0, Ny, Nx = dev_tables(p, dev)
            S = N * p.ny * p.nx
            for guided in (False, True):
                B = 2 * S if guided else S
                x = rnd(N, HC, WC, Cc)
                # gather: the stream, pre-filled with NaN patterns, is fully overwritten and equals the canvas under the map
                img = nan(B, WH * WW, Cc).to(dev)
                assert torch.isnan(img.float()).all()
                xd = x.to(dev)
                ops.window_gather(xd, img, row0, col0, WH, WW, guided=guided)
                torch.cuda.synchronize()
                want = wr.gather(x, p.row0, p.col0, WH, WW, guided=guided)
                assert not torch.isnan(img.float()).any(), "gather left a stream element unwritten"
                assert torch.equal(img.cpu(), want) and torch.equal(xd.cpu(), x), f"gather C={Cc} {profile} guided={guided}"
                for j in (0, 2):
                    pred = rnd(B, WH * WW, Cc)
                    xd, img, pd = x.to(dev), nan(B, WH * WW, Cc).to(dev), pred.to(dev)
                    step = torch.tensor([j], dtype=torch.int32, device=dev)
                    ops.window_step(xd, img, pd, dts, row0, col0, Ny, Nx, WH, WW, step=step, scale=sc if guided else None)
                    torch.cuda.synchronize()
                    want_x, want_img = wr.step(x, pred, f32(DTS[j]), p.row0, p.col0, p.Ny, p.Nx, WH, WW, scale=SCALE if guided else None)
                    tag = f"C={Cc} {profile} guided={guided} step={j}"
                    assert torch.equal(xd.cpu(), want_x), f"{tag}: canvas rel-L2 {rel_l2(xd, want_x):.3e}"
                    assert not torch.isnan(img.float()).any(), f"{tag}: step left a stream element unwritten"
                    assert torch.equal(img.cpu(), want_img), f"{tag}: stream rel-L2 {rel_l2(img, want_img):.3e}"
                    assert torch.equal(pd.cpu(), pred), f"{tag}: pred changed"
                    if guided:  # the canvas and both halves of the stream agree
                        assert torch.equal(img[:S], img[S:]) and torch.equal(img[:S].cpu(), wr.gather(want_x, p.row0, p.col0, WH, WW))
                    if j == 0:  # step == NULL reads row 0
                        xd2, img2 = x.to(dev), torch.zeros_like(img)
                        ops.window_step(xd2, img2, pd, dts, row0, col0, Ny, Nx, WH, WW, scale=sc if guided else None)
                        torch.cuda.synchronize()
                        assert torch.equal(xd2, xd) and torch.equal(img2, img)


@pytest.mark.parametrize("N", [1, 2])
def test_one_window_is_the_euler_step(dev, N):
    """the canvas equal to the window: fluxmi_euler (guided: fluxmi_cfg_euler) bit for bit, whatever the profile"""
    from fluxmi import ops

    g = torch.Generator().manual_seed(7 + N)
    rnd = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).to(dev)
    dt = DTS[0]
    dts = torch.tensor([dt], dtype=torch.float32, device=dev)
    sc = torch.tensor([SCALE], dtype=torch.float32, device=dev)
    for profile in ("cosine", "uniform"):
        p = make_plan((1, 1), profile, Hc=WH, Wc=WW)
        assert (p.ny, p.nx) == (1, 1)
        row0, col0, Ny, Nx = dev_tables(p, dev)
        x, pred = rnd(N, WH, WW, 64), rnd(N, WH * WW, 64)
        a, img = x.clone(), torch.zeros_like(pred)
        ops.window_step(a, img, pred, dts, row0, col0, Ny, Nx, WH, WW)
        b = ops.euler_(x.clone().view(N, WH * WW, 64), pred, dt)
        torch.cuda.synchronize()
        assert torch.equal(a.view_as(b), b) and torch.equal(img, b)
        pred2 = rnd(2 * N, WH * WW, 64)
        a, img = x.clone(), torch.zeros_like(pred2)
        ops.window_step(a, img, pred2, dts, row0, col0, Ny, Nx, WH, WW, scale=sc)
        xx = x.view(N, WH * WW, 64)
        b = ops.cfg_euler(torch.cat((xx, xx), 0).contiguous(), pred2, dt, SCALE)
        torch.cuda.synchronize()
        assert torch.equal(img, b) and torch.equal(a.view(N, WH * WW, 64), b[:N]) and torch.equal(b[:N], b[N:])


def test_window_kernel_refusals(dev):
    from fluxmi import _lib, ops

    p = make_plan()
    row0, col0, Ny, Nx = dev_tables(p, dev)
    N, Cc = 1, 64
    S = N * p.ny * p.nx
    x = torch.randn(N, HC, WC, Cc).to(torch.bfloat16).to(dev)
    img, pred = torch.zeros(S, WH * WW, Cc, dtype=torch.bfloat16, device=dev), torch.ones(S, WH * WW, Cc, dtype=torch.bfloat16, device=dev)
    dts = torch.tensor(DTS, dtype=torch.float32, device=dev)
    x_kept = x.clone()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)

    def step_args(**k):
        r, c = k.get("row0", row0), k.get("col0", col0)
        return [ops._p(x), ops._p(img), ops._p(pred), ops._p(dts), None, None, None if r is None else ops._p(r), None if c is None else ops._p(c),
                ops._p(Ny) if k.get("Ny", True) else None, ops._p(Nx) if k.get("Nx", True) else None, k.get("N", N), k.get("Hc", HC), k.get("Wc", WC),
                k.get("h", WH), k.get("w", WW), k.get("ny", p.ny), k.get("nx", p.nx), k.get("C", Cc), ops._stream()]

    def gather_args(**k):
        a = step_args(**k)
        return a[:2] + a[6:8] + a[10:18] + [0, a[18]]

    cases = [
        (dict(C=60), "C=60"),
        (dict(h=HC + 1), "leaves the canvas|inside the canvas"),
        (dict(w=WC + 1), "leaves the canvas|inside the canvas"),
        (dict(row0=i32([0, 3])), "leaves the canvas"),          # 3 + 4 > 6
        (dict(col0=i32([0, 3, 7])), "leaves the canvas"),
        (dict(row0=i32([-1, 2])), "leaves the canvas"),
        (dict(col0=i32([0, 1, 2])), "under no window"),          # columns 6 .. 9 uncovered
        (dict(row0=i32([0, 0])), "under no window"),
        (dict(col0=i32([0, 6, 6])), "under no window"),          # a gap in the middle: columns 4, 5
        (dict(row0=None), "NULL tables"),
        (dict(col0=None), "NULL tables"),
        (dict(N=1 << 24, Hc=16, Wc=16, h=16, w=16, ny=1, nx=1), "32-bit index"),  # 2^24 * 256 tokens * 8 vectors
    ]
    for k, match in cases:
        with pytest.raises(RuntimeError, match=match):
            _lib.call("fluxmi_window_step", *step_args(**k))
        with pytest.raises(RuntimeError, match=match):
            _lib.call("fluxmi_window_gather", *gather_args(**k))
    for k in (dict(Ny=False), dict(Nx=False)):
        with pytest.raises(RuntimeError, match="NULL tables"):
            _lib.call("fluxmi_window_step", *step_args(**k))
    # the stream counts too: 2S samples of a guided call
    with pytest.raises(RuntimeError, match="32-bit index"):
        a = step_args(N=1 << 16, Hc=64, Wc=64, h=64, w=64, ny=1, nx=1)  # 2^16 * 4096 * 8 = 2^31 canvas vectors
        _lib.call("fluxmi_window_step", *a)
    torch.cuda.synchronize()
    assert torch.equal(x, x_kept) and (img == 0).all(), "a refused call wrote"
    assert _lib.lib.fluxmi_window_step(*step_args(C=60)) != 0 and "window_step" in _lib.lib.fluxmi_last_error().decode()


# ---- engine helpers -----------------------------------------------------------------------------------------------------------------------
def win_inputs(params, N, seed, dev, Hc=HC, Wc=WC, h=WH, w=WW):
    """the helpers' 64 x 64 inputs give the text, y and the WINDOW's position ids; the canvas is drawn here"""
    d = to_dev(inputs("plain", params, 16 * h, 16 * w, 32, N, seed=seed), dev)
    g = torch.Generator().manual_seed(900 + seed)
    d["canvas"] = torch.randn(N, Hc, Wc, 64, generator=g).to(torch.bfloat16).to(dev)
    d["win_ids"] = d["img_ids"][:1]
    return d


def run_windows(model, d, p, ts, canvas=None, guided=False, use_graph=True, scale=SCALE, **kw):
    neg = dict(neg_txt=d["neg_txt"], neg_y=d["neg_y"], cfg_scale=scale) if guided else {}
    return model.denoise_windows(d["canvas"] if canvas is None else canvas, p, d["win_ids"], d["txt"], d["txt_ids"], d["y"], ts, guidance=3.5,
                                 use_graph=use_graph, **neg, **kw)


def python_window_loop(model, d, p, ts, canvas, guided, mode=None, scale=SCALE):
    """fluxmi_engine_forward (Flux.forward) on the gathered windows, then the C-entry kernel, per step"""
    from fluxmi import ops

    dev, N = canvas.device, canvas.shape[0]
    per = p.ny * p.nx
    S = N * per
    B = 2 * S if guided else S
    row0, col0, Ny, Nx = dev_tables(p, dev)
    rep = lambda t: t.expand(N, *t.shape[1:]).repeat_interleave(per, 0)
    txt, y = rep(d["txt"]), rep(d["y"])
    if guided:
        txt, y = torch.cat((txt, rep(d["neg_txt"])), 0), torch.cat((y, rep(d["neg_y"])), 0)
    ids, tids = d["win_ids"].expand(B, -1, -1).contiguous(), d["txt_ids"][:1].expand(B, -1, -1).contiguous()
    g = torch.full((B,), 3.5, dtype=torch.bfloat16, device=dev)
    x = canvas.clone()
    img = torch.empty(B, p.h * p.w, canvas.shape[3], dtype=torch.bfloat16, device=dev)
    ops.window_gather(x, img, row0, col0, p.h, p.w, guided=guided)
    dts = torch.tensor([b - a for a, b in zip(ts[:-1], ts[1:])], dtype=torch.float32, device=dev)
    sc = torch.tensor([scale], dtype=torch.float32, device=dev) if guided else None
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    for j, t in enumerate(ts[:-1]):
        tv = torch.full((B,), t, dtype=torch.bfloat16, device=dev)
        pred = model(img, ids, txt, tids, tv, y, g, mode=mode).contiguous()
        step.fill_(j)
        ops.window_step(x, img, pred, dts, row0, col0, Ny, Nx, p.h, p.w, step=step, scale=sc)
    return x


# ---- 2. engine: graph == eager == python loop, through calibration ------------------------------------------------------------------------
@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "guided"])
@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_window_denoise_bit_exact(dev, qname, guided):
    """canvas 96 x 160 px, windows 64 x 64 at overlap 16: S = 6.  17 steps from a fresh model: fp8 runs 13 calibrating steps (one trial each)
    and 4 replayed ones; three models of the same weights run the graph loop, the eager loop and the python loop"""
    cfg = tiny_config()
    p = make_plan((3, 3))
    assert (p.row0, p.col0) == ([0, 2], [0, 3, 6])
    ts = fo.get_schedule(17, WH * WW)
    out = []
    for how in ("graph", "eager", "python"):
        model, _ = build(cfg, QUANTS[qname], dev)
        d = win_inputs(cfg.params, 1, 5, dev)
        kept = d["canvas"].clone()
        if how == "python":
            out.append(python_window_loop(model, d, p, ts, d["canvas"], guided))
        else:
            out.append(run_windows(model, d, p, ts, guided=guided, use_graph=how == "graph"))
        if qname == "fp8":
            assert model.calibration_state()[0], f"{how}: 17 steps did not freeze the scales"
        assert torch.equal(d["canvas"], kept), "the caller's canvas changed"
    a, b, c = out
    assert a.shape == kept.shape and a.dtype == torch.bfloat16 and torch.isfinite(a).all() and not torch.equal(a, kept)
    assert torch.equal(a, b), f"graph vs eager: rel-L2 {rel_l2(a, b):.3e}"
    assert torch.equal(a, c), f"graph loop vs python loop: rel-L2 {rel_l2(a, c):.3e}"
    # the frozen model again: graph == eager == python loop, and the other kind differs
    ts2 = ts[4:9]
    a2 = run_windows(model, d, p, ts2, canvas=a, guided=guided)
    assert torch.equal(a2, run_windows(model, d, p, ts2, canvas=a, guided=guided, use_graph=False))
    assert torch.equal(a2, python_window_loop(model, d, p, ts2, a, guided, mode=1 if qname == "fp8" else 2))
    assert not torch.equal(a2, run_windows(model, d, p, ts2, canvas=a, guided=not guided)), "the negative branch has no effect"
    # a request cut into two denoise calls equals the uncut one
    head = run_windows(model, d, p, ts2[:3], canvas=a, guided=guided)
    assert torch.equal(a2, run_windows(model, d, p, ts2[2:], canvas=head, guided=guided)), "2 + 2 steps differ from 4"


@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_plain_guided_and_windowed_requests_never_share_a_graph(dev, qname):
    """one prepared shape (six samples of 16 rows): plain B = 6, guided B = 3, windowed S = 6, in turn"""
    cfg = tiny_config()
    model, _ = build(cfg, QUANTS[qname], dev)
    d6 = to_dev(inputs("plain", cfg.params, 64, 64, 32, 6, seed=5), dev)
    d3 = {k: v[:3] for k, v in d6.items()}
    dw = win_inputs(cfg.params, 1, 5, dev)
    p, pu, pt = make_plan((3, 3)), make_plan((3, 3), "uniform"), make_plan((3, 3), Hc=WC, Wc=HC)
    ts = fo.get_schedule(16, WH * WW)
    lat = plain_denoise(model, d6, ts[:14], use_graph=False)
    ts2 = ts[:7]
    runs = [lambda: plain_denoise(model, d6, ts2, img=lat), lambda: guided_denoise(model, d3, ts2, img=lat[:3]),
            lambda: run_windows(model, dw, p, ts2)]
    first = []
    for r in runs:
        c0 = captures(model)
        first.append(r())
        assert captures(model) > c0, "a request of another kind replayed the previous kind's graph"
    for _ in range(2):
        for i, r in enumerate(runs):
            c0 = captures(model)
            again = r()
            assert captures(model) > c0, f"request kind {i} replayed another kind's graph"
            assert torch.equal(first[i], again), f"request kind {i} differs from its own first result: rel-L2 {rel_l2(again, first[i]):.3e}"
    # tables, weights, scale and schedule are device data: one graph serves them; the canvas geometry is part of the key
    c0 = captures(model)
    assert torch.equal(run_windows(model, dw, p, ts2), first[2]) and captures(model) == c0, "the same windowed request re-captured"
    other = run_windows(model, dw, pu, ts[1:8])
    assert captures(model) == c0 and not torch.equal(other, first[2]), "other weights and times re-captured the step graph"
    shifted = run_windows(model, dw, make_plan((3, 4)), ts2)  # the same grid of windows at other positions (columns 0, 4, 6)
    assert captures(model) == c0 and not torch.equal(shifted, first[2])
    turned = run_windows(model, {**dw, "canvas": dw["canvas"].transpose(1, 2).contiguous()}, pt, ts2)
    assert captures(model) > c0 and tuple(turned.shape) == (1, WC, HC, 64), "another canvas geometry replayed the old graph"
    assert torch.equal(run_windows(model, dw, p, ts2), first[2])
    assert torch.equal(python_window_loop(model, dw, p, ts2, dw["canvas"], False, mode=1 if qname == "fp8" else 2), first[2])
    # two images: windows of image 1 are samples 6 .. 11; an image does not depend on its batch
    dw2 = win_inputs(cfg.params, 2, 5, dev)
    both = run_windows(model, dw2, p, ts2)
    one = run_windows(model, {k: v[1:2] if k != "win_ids" else v for k, v in dw2.items()}, p, ts2)
    assert torch.equal(both[1], one[0]), f"an image depends on its batch: rel-L2 {rel_l2(both[1], one[0]):.3e}"


def test_engine_refusals_and_hook(dev):
    from fluxmi import GenerationCancelled, _lib, ops
    from modules.flux_model import PreviewCall

    cfg = tiny_config()
    model, _ = build(cfg, None, dev)
    d = win_inputs(cfg.params, 1, 3, dev)
    p = make_plan((3, 3))
    ts = fo.get_schedule(8, WH * WW)[:5]
    want = run_windows(model, d, p, ts)
    # a hook with every = 0: progress, then cancellation
    seen = []
    got = run_windows(model, d, p, ts, preview=PreviewCall(None, (0, 0), 0, 0, 4, lambda e, n, rgb: seen.append((e, n, rgb)) or True))
    assert torch.equal(got, want) and seen == [(0, 4, None), (1, 4, None), (2, 4, None), (3, 4, None)]
    with pytest.raises(GenerationCancelled):
        run_windows(model, d, p, ts, preview=PreviewCall(None, (0, 0), 0, 0, 4, lambda e, n, rgb: e < 1))
    with pytest.raises(ValueError, match="no previews"):
        run_windows(model, d, p, ts, preview=PreviewCall([0.0] * 51, (WH, WW), 1, 0, 4, lambda e, n, rgb: True))
    with pytest.raises(ValueError, match="one engine pass"):
        run_windows(model, win_inputs(cfg.params, 6, 3, dev), p, ts)  # 36 windows
    with pytest.raises(ValueError, match="one engine pass"):
        run_windows(model, win_inputs(cfg.params, 3, 3, dev), p, ts, guided=True)  # 2 x 18
    assert torch.equal(run_windows(model, d, p, ts), want)
    # the C entries: no state, a state that does not fit the prepared shape, workspace accounting
    t_io, tsc = C.c_int(0), (C.c_double * len(ts))(*ts)
    B = p.ny * p.nx
    txt, y = d["txt"].expand(B, -1, -1).contiguous(), d["y"].expand(B, -1).contiguous()
    canvas = d["canvas"].clone()
    call = lambda guided=0: _lib.call("fluxmi_engine_denoise_windows", model._engine, ops._p(canvas), ops._p(txt), ops._p(y), 3.5, guided, SCALE, tsc,
                                      len(ts) - 1, C.byref(t_io), 1, ops._stream())
    row0, col0 = (C.c_int * p.ny)(*p.row0), (C.c_int * p.nx)(*p.col0)
    wy, wx = (C.c_float * (p.ny * HC))(*p.Ny.reshape(-1).tolist()), (C.c_float * (p.nx * WC))(*p.Nx.reshape(-1).tolist())
    set_w = lambda **k: _lib.call("fluxmi_engine_set_windows", model._engine, k.get("N", 1), HC, WC, k.get("h", WH), WW, p.ny, p.nx,
                                  k.get("row0", row0), col0, wy, wx, ops._stream())
    with model._lock:  # the engine is still prepared for this request's six samples
        bytes0 = C.c_longlong(0)
        with pytest.raises(RuntimeError, match="no window state is set"):
            call()
        _lib.call("fluxmi_engine_workspace_bytes", model._engine, C.byref(bytes0))
        with pytest.raises(RuntimeError, match="do not fit the prepared batch"):
            set_w(N=2)
        with pytest.raises(RuntimeError, match="image rows"):
            set_w(h=3)
        with pytest.raises(RuntimeError, match="leaves the canvas"):
            set_w(row0=(C.c_int * 2)(0, 3))
        with pytest.raises(RuntimeError, match="under no window"):
            set_w(row0=(C.c_int * 2)(0, 0))
        set_w()
        with pytest.raises(RuntimeError, match="prepared shape"):
            call(guided=1)  # 2S = 12 samples are not prepared
        call()
        torch.cuda.synchronize()
        assert torch.equal(canvas, want)
        _lib.call("fluxmi_engine_set_step_cache", model._engine, 0.1, 0)
        with pytest.raises(RuntimeError, match="step caching"):
            call()
        _lib.call("fluxmi_engine_set_step_cache", model._engine, 0.0, 0)
        _lib.call("fluxmi_engine_set_windows", model._engine, 0, 0, 0, 0, 0, 0, 0, None, None, None, None, None)
        with pytest.raises(RuntimeError, match="no window state is set"):
            call()
    assert torch.equal(run_windows(model, d, p, ts), want)


# ---- 3. pipeline --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe(dev):
    pl = tiny_pipeline(dev)
    pl.compile()
    assert pl.model.calibration_state()[0]
    return pl


def test_pipeline_tiled(dev, pipe):
    import numpy as np

    from fluxmi import GenerationCancelled

    pos, neg = prompts()
    H, W, n = 96, 160, 6
    kw = dict(width=W, height=H, num_steps=n, seed=7, silent=True, output_type="latent")
    tiled = dict(kw, tile_size=64, tile_overlap=16)
    plain_kw = dict(width=64, height=96, num_steps=n, seed=7, silent=True, output_type="latent")
    plain_before = pipe.generate(pos, **plain_kw)
    a = pipe.generate(pos, **tiled)
    assert tuple(a.shape) == (1, 16, 12, 20) and torch.isfinite(a).all()
    assert torch.equal(a, pipe.generate(pos, **tiled)), "same seed, different latents"
    # == the python loop on the same noise, with the WINDOW's schedule
    p = make_plan((3, 3))
    gen, _ = pipe.set_seed(7)
    x, ts = pipe.preprocess_latent(height=H, width=W, num_steps=n, generator=gen, image_seq_len=WH * WW)
    assert ts == pipe.get_schedule(n, WH * WW) and ts != pipe.get_schedule(n, HC * WC)
    img, _, vec, txt, txt_ids = map(lambda t: t.contiguous(), pipe.prepare(x, pos))
    d = dict(txt=txt, y=vec, txt_ids=txt_ids, win_ids=pipe.make_img_ids(1, WH, WW, dev, pipe.dtype))
    _, _, nvec, ntxt, _ = pipe.prepare(x, neg)
    d.update(neg_txt=ntxt, neg_y=nvec)
    canvas = img.reshape(1, HC, WC, 64).to(torch.bfloat16)
    want = python_window_loop(pipe.model, d, p, ts, canvas, False)
    assert torch.equal(a, pipe.unpack(want.reshape(1, HC * WC, 64).float(), H, W)), "generate differs from the python loop on the same noise"
    assert not torch.equal(a, pipe.generate(pos, **kw)), "the tiled request equals the untiled one"
    assert not torch.equal(a, pipe.generate(pos, **dict(tiled, tile_weight="uniform")))
    assert torch.equal(pipe.generate(pos, **dict(kw, tile_size=(64, 64))), a), "the default overlap of a 64 px tile is 16 px"
    # one tile of the request's size is today's request, bit for bit
    one = dict(width=64, height=64, num_steps=n, seed=7, silent=True, output_type="latent")
    c0 = captures(pipe.model)
    base = pipe.generate(pos, **one)
    assert torch.equal(pipe.generate(pos, tile_size=64, **one), base)
    # ... and through the windowed path (another tile argument given) one window is still the Euler step
    assert torch.equal(pipe.generate(pos, tile_size=64, tile_weight="uniform", **one), base)
    # a negative prompt, and an interval of it: up to three denoise calls on the canvas
    gkw = dict(tiled, negative_prompt=neg, true_cfg_scale=SCALE)
    ga = pipe.generate(pos, **gkw)
    wg = python_window_loop(pipe.model, d, p, ts, canvas, True)
    assert torch.equal(ga, pipe.unpack(wg.reshape(1, HC * WC, 64).float(), H, W)) and not torch.equal(ga, a)
    gi = pipe.generate(pos, **dict(gkw, true_cfg_interval=(0.0, 0.5)))
    w3 = python_window_loop(pipe.model, d, p, ts[3:], python_window_loop(pipe.model, d, p, ts[:4], canvas, True), False)
    assert torch.equal(gi, pipe.unpack(w3.reshape(1, HC * WC, 64).float(), H, W))
    # num_images: twelve windows in one pass, each image on its own noise
    two = pipe.generate(pos, **dict(tiled, num_images=2))
    gen, _ = pipe.set_seed(7)
    xx, _ = pipe.preprocess_latent(height=H, width=W, num_steps=n, generator=gen, num_images=2, image_seq_len=WH * WW)
    w2 = python_window_loop(pipe.model, d, p, ts, pipe.pack(xx).reshape(2, HC, WC, 64).to(torch.bfloat16), False)
    assert two.shape[0] == 2 and torch.equal(two, pipe.unpack(w2.reshape(2, HC * WC, 64).float(), H, W)) and not torch.equal(two[0], two[1])
    # on_step: progress and cancellation
    seen = []
    assert torch.equal(pipe.generate(pos, on_step=lambda info: seen.append(info) or True, **gkw), ga)
    assert [i["evaluation"] for i in seen] == list(range(n)) and all(i["num_evaluations"] == n and i["preview"] is None for i in seen)
    with pytest.raises(GenerationCancelled):
        pipe.generate(pos, on_step=lambda info: info["evaluation"] < 1, **tiled)
    # init_image at strength 0.5 starts from the canvas-sized encoded image, on the truncated window schedule
    photo = np.random.default_rng(0).integers(0, 256, size=(120, 200, 3), dtype=np.uint8)
    torch.manual_seed(11)
    got = pipe.generate(pos, init_image=photo, strength=0.5, **tiled)
    torch.manual_seed(11)
    gen, _ = pipe.set_seed(7)
    x2, ts_i, lat, noise = pipe.preprocess_latent_parts(init_image=pipe.load_init_image_if_needed(photo), height=H, width=W, num_steps=n,
                                                        strength=0.5, generator=gen, image_seq_len=WH * WW)
    assert tuple(lat.shape) == (1, 16, H // 8, W // 8) and ts_i == ts[n // 2:] and torch.equal(noise, x)
    assert torch.equal(x2, ts_i[0] * noise + (1.0 - ts_i[0]) * lat)
    c2 = pipe.pack(x2).reshape(1, HC, WC, 64).to(torch.bfloat16)
    wi = python_window_loop(pipe.model, d, p, ts_i, c2, False)
    assert torch.equal(got, pipe.unpack(wi.reshape(1, HC * WC, 64).float(), H, W)) and not torch.equal(got, a)
    # through the VAE at canvas size
    px = torch.as_tensor(pipe.generate(pos, **dict(tiled, output_type="uint8")))
    assert px.dtype == torch.uint8 and tuple(px.shape) == (1, H, W, 3) and px.float().std() > 0
    # a request without tile arguments is bit-identical before and after
    assert torch.equal(pipe.generate(pos, **plain_kw), plain_before)
    assert torch.equal(pipe.generate(pos, **tiled), a)


# ---- 4. against the oracle ------------------------------------------------------------------------------------------------------------------
def oracle_window_loop(oracle, inp, canvas, p, ts, guidance=3.5):
    """FluxOracle.forward per step on the S windows, each a stand-alone image, blended by window_ref on the CPU"""
    S = canvas.shape[0] * p.ny * p.nx
    ex = lambda t: t[:1].expand(S, *t.shape[1:]).contiguous()
    g = torch.full((S,), guidance, dtype=oracle.dtype)
    x = canvas.to(torch.bfloat16)
    img = wr.gather(x, p.row0, p.col0, p.h, p.w)
    for t_curr, t_prev in zip(ts[:-1], ts[1:]):
        tv = torch.full((S,), t_curr, dtype=oracle.dtype)
        pred = oracle.forward(img, ex(inp["img_ids"]), ex(inp["txt"]), ex(inp["txt_ids"]), tv, ex(inp["y"]), g).to(torch.bfloat16)
        x, img = wr.step(x, pred, f32(t_prev - t_curr), p.row0, p.col0, p.Ny, p.Nx, p.h, p.w)
    return x


def test_window_denoise_matches_oracle(dev, monkeypatch):
    """N = 1, canvas 96 x 160 px, S = 6 windows of 64 x 64, Lt 32, 4 steps.  The gates are those of
    test_flowedit_gpu.test_edit_denoise_matches_oracle, on the canvas:
      fp8 flows: rel-L2(engine, oracle-bf16) <= 1.25 x rel-L2(oracle-fp8, oracle-bf16)                         (the project's gate (iv));
      bf16 flow: rel-L2(engine, oracle-bf16) <= max(1e-2, 1.75 x floor), floor = the bf16 oracle's own movement under fo.attention_exact."""
    p = make_plan((3, 3))
    ts = fo.get_schedule(4, WH * WW)
    ref = {}
    for qname in QUANTS:
        cfg = tiny_config()
        model, sd = build(cfg, QUANTS[qname], dev)
        inp = inputs("plain", cfg.params, 64, 64, 32, 1, seed=7)
        canvas = torch.randn(1, HC, WC, 64, generator=torch.Generator().manual_seed(907)).to(torch.bfloat16)
        if not ref:
            ref["o16"] = oracle_window_loop(make_oracle(cfg, sd, None), inp, canvas, p, ts)
            with monkeypatch.context() as mp:
                mp.setattr(fo, "attention", fo.attention_exact)
                ref["o16x"] = oracle_window_loop(make_oracle(cfg, sd, None), inp, canvas, p, ts)
            ref["floor16"] = rel_l2(ref["o16x"], ref["o16"])
        d = to_dev(inp, dev)
        d.update(canvas=canvas.to(dev), win_ids=d["img_ids"][:1])
        got = run_windows(model, d, p, ts)
        assert got.shape == canvas.shape and torch.isfinite(got).all()
        e16 = rel_l2(got, ref["o16"])
        if qname == "bf16":
            gate = max(1e-2, 1.75 * ref["floor16"])
            print(f"[windows bf16] engine vs oracle-bf16 {e16:.3e}; floor (oracle-bf16, exact attention) {ref['floor16']:.3e}; gate {gate:.3e}; "
                  f"ratio to the gate {e16 / gate:.3f}")
            assert e16 <= gate, f"bf16: rel-L2 {e16:.3e} > max(1e-2, 1.75 x {ref['floor16']:.3e})"
        else:
            o8 = oracle_window_loop(make_oracle(cfg, sd, QUANTS[qname]), inp, canvas, p, ts)
            yard = rel_l2(o8, ref["o16"])
            print(f"[windows {qname}] engine vs oracle-bf16 {e16:.3e}; yardstick (oracle-fp8 vs oracle-bf16) {yard:.3e}; ratio {e16 / yard:.3f} "
                  f"(gate 1.25); engine vs oracle-fp8 {rel_l2(got, o8):.3e}")
            assert e16 <= 1.25 * yard, f"{qname}: vs bf16 flow {e16:.3e} > 1.25 x {yard:.3e}"


# ---- 5. real width -----------------------------------------------------------------------------------------------------------------------
def test_windows_at_real_width(dev):
    """hidden 3072, 1 + 1 blocks, canvas 2048 x 1024 px, windows 1024^2 at overlap 256 (columns 0, 768, 1024 px: three windows, the last
    snapped), Lt 512, 3 evaluations on a frozen model: graph == eager, finite"""
    import util

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    cfg.params.depth, cfg.params.depth_single_blocks = 1, 1
    model, _ = build(cfg, QUANTS["fp8"], dev, seed=2)
    p = make_plan((48, 48), Hc=64, Wc=128, h=64, w=64)
    assert (p.row0, p.col0) == ([0], [0, 48, 64])
    d = to_dev(inputs("plain", cfg.params, 1024, 1024, 512, 1, seed=8, real_tokens=64), dev)
    d["canvas"] = torch.randn(1, 64, 128, 64, generator=torch.Generator().manual_seed(908)).to(torch.bfloat16).to(dev)
    d["win_ids"] = d["img_ids"][:1]
    assert d["win_ids"].shape[1] + 512 == 4608
    ts = fo.get_schedule(16, 4096)
    lat = run_windows(model, d, p, ts[:14], use_graph=False)  # calibrate at this shape
    assert model.calibration_state()[0] and torch.isfinite(lat).all()
    ts2 = ts[4:8]
    a = run_windows(model, d, p, ts2, canvas=lat)
    b = run_windows(model, d, p, ts2, canvas=lat, use_graph=False)
    assert torch.isfinite(a).all() and torch.equal(a, b), f"graph vs eager: rel-L2 {rel_l2(a, b):.3e}"
    assert not torch.equal(a, lat)
    print(f"[windows 2048 x 1024, S=3] graph == eager; canvas std {a.float().std().item():.3f}")
