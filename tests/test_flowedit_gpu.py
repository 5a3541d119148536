"""FlowEdit on the GPU (include/fluxmi.h: fluxmi_flowedit_couple / _step, fluxmi_engine_set_flow_edit / _denoise_edit).
The image stream of an edit request holds 2B samples -- the source branches, then the target branches of the same images, with DIFFERENT
latents -- and the edit state z lives beside it.  Kernel and engine are checked bit for bit against tests/flowedit_ref.py's bf16 chain fed
the normals fluxmi_philox_normal returns; the oracle loop is FluxOracle.forward on the two-sample batch plus that chain.  Model helpers are
those of tests/test_cfg_gpu.py (hidden 256, 2 + 2 blocks, 64 x 64 pixels, Lt 32)."""
import ctypes as C
import io

import pytest
import torch

import flowedit_ref as fr
import flux_oracle as fo
from test_cfg_gpu import KNOB_SETS, QUANTS, build, dup, guided_denoise, inputs, make_oracle, plain_denoise, prompts, rel_l2, tiny_config, tiny_pipeline, to_dev

pytestmark = pytest.mark.gpu

GS, GT = 1.5, 5.5  # source / target distilled guidance
IDS3 = [(0xa4093822, 0x299f31d0, 0, 1), (0xa4093822, 0x299f31d0, 1, 1), (0x00000007, 0xffffffff, 2, 1)]


def ids_tensor(ids, dev):
    return torch.tensor([[w if w < 2 ** 31 else w - 2 ** 32 for w in row] for row in ids], dtype=torch.int32, device=dev).contiguous()


def normals(dev, ids, shape, ev):
    """fluxmi_philox_normal -> fp32 [B, *shape]: the draw of index `ev`"""
    from fluxmi import _lib, ops

    n = 1
    for s in shape:
        n *= s
    out = torch.full((len(ids), n), float("nan"), dtype=torch.float32, device=dev)
    _lib.call("fluxmi_philox_normal", ops._p(out), ops._p(ids_tensor(ids, dev)), len(ids), n, ev, 0, ops._stream())
    torch.cuda.synchronize()
    return out.view(len(ids), *shape)


def tables(program, dev):
    return (torch.tensor(program.coef, dtype=torch.float32, device=dev).reshape(-1, 4).contiguous(),
            torch.tensor(program.ctl, dtype=torch.int32, device=dev).reshape(-1, 2).contiguous())


# ---- 1. the kernel against the torch restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_flowedit_kernels_bit_exact(dev, B):
    from fluxmi import _lib, flowedit, ops

    R, Cc = 15, 64  # odd rows: 120 vectors per image, no multiple of the block
    ids = IDS3[:B]
    g = torch.Generator().manual_seed(40 + B)
    rnd = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).to(dev)
    x0, z = rnd(B, R, Cc), rnd(B, R, Cc)
    x0_kept, z_kept = x0.clone(), z.clone()
    for t, ev in ((0.8125, 0), (0.3, 7), (1.0, 2 ** 31 - 1)):
        out = ops.flowedit_couple(z, x0, t, ids, ev)
        torch.cuda.synchronize()
        zs, zt = fr.couple_bf16(z, x0, t, 1.0 - t, normals(dev, ids, (R, Cc), ev))
        assert torch.equal(out[:B], zs), f"couple t={t}: source half rel-L2 {rel_l2(out[:B], zs):.3e}"
        assert torch.equal(out[B:], zt), f"couple t={t}: target half rel-L2 {rel_l2(out[B:], zt):.3e}"
        assert torch.equal(z, z_kept) and torch.equal(x0, x0_kept)
    ts = [1.0, 0.8125, 0.59375, 0.3125]
    for n_avg, rows in ((1, (0, 2)), (3, (0, 1, 2))):  # n_avg 3: a first row, a middle row and an apply row
        prog = flowedit.build_program(ts, n_avg)
        coef, ctl = tables(prog, dev)
        for j in rows:
            for off in (0, 5):
                img = rnd(2 * B, R, Cc)
                pred, zz = rnd(2 * B, R, Cc), rnd(B, R, Cc)
                acc = torch.randn(B, R, Cc, generator=g).to(dev) if n_avg > 1 else None
                pred_kept, acc_kept = pred.clone(), None if acc is None else acc.clone()
                want_img, want_z, want_acc = fr.step_bf16(pred, zz, acc, x0, prog.coef[j], prog.ctl[j], normals(dev, ids, (R, Cc), j + 1 + off))
                step, offt = torch.tensor([j], dtype=torch.int32, device=dev), torch.tensor([off], dtype=torch.int32, device=dev)
                ops.flowedit_step(img, pred, zz, x0, coef, ctl, ids, acc=acc, step=step, eval_offset=offt)
                torch.cuda.synchronize()
                tag = f"n_avg={n_avg} row={j} off={off}"
                assert torch.equal(zz, want_z), f"{tag}: z rel-L2 {rel_l2(zz, want_z):.3e}"
                assert torch.equal(img[:B], want_img[:B]), f"{tag}: source half rel-L2 {rel_l2(img[:B], want_img[:B]):.3e}"
                assert torch.equal(img[B:], want_img[B:]), f"{tag}: target half rel-L2 {rel_l2(img[B:], want_img[B:]):.3e}"
                if acc is not None:  # stored by a row without apply, untouched by an apply row
                    assert torch.equal(acc, acc_kept if prog.ctl[j][1] else want_acc), f"{tag}: acc"
                assert torch.equal(pred, pred_kept) and torch.equal(x0, x0_kept), f"{tag}: pred or x0 changed"
    # step = NULL and eval_offset = NULL read row 0 and draw at 1
    prog = flowedit.build_program(ts, 1)
    coef, ctl = tables(prog, dev)
    img, pred, zz = rnd(2 * B, R, Cc), rnd(2 * B, R, Cc), rnd(B, R, Cc)
    want_img, want_z, _ = fr.step_bf16(pred, zz, None, x0, prog.coef[0], prog.ctl[0], normals(dev, ids, (R, Cc), 1))
    ops.flowedit_step(img, pred, zz, x0, coef, ctl, ids)
    torch.cuda.synchronize()
    assert torch.equal(zz, want_z) and torch.equal(img, want_img)
    # refusals
    d_ids, s = ids_tensor(ids, dev), ops._stream
    args = lambda **k: [ops._p(img), ops._p(pred), ops._p(zz), k.get("acc"), ops._p(x0), ops._p(coef), ops._p(k.get("ctl", ctl)), k.get("step"),
                        k.get("ids", ops._p(d_ids)), None, B, k.get("img_rows", R), k.get("pred_rows", R), k.get("c_in", Cc), k.get("c_out", Cc), s()]
    for bad in (dict(c_in=128), dict(pred_rows=R - 1), dict(img_rows=R + 9)):
        with pytest.raises(RuntimeError, match="FlowEdit steps the whole stream"):
            _lib.call("fluxmi_flowedit_step", *args(**bad))
        with pytest.raises(RuntimeError, match="FlowEdit steps the whole stream"):
            _lib.call("fluxmi_flowedit_couple", ops._p(img), ops._p(zz), ops._p(x0), 0.5, 0.5, ops._p(d_ids), 0, B, bad.get("img_rows", R),
                      bad.get("pred_rows", R), bad.get("c_in", Cc), Cc, s())
    with pytest.raises(RuntimeError, match="NULL ids"):
        _lib.call("fluxmi_flowedit_step", *args(ids=None))
    with pytest.raises(RuntimeError, match="NULL ids"):
        _lib.call("fluxmi_flowedit_couple", ops._p(img), ops._p(zz), ops._p(x0), 0.5, 0.5, None, 0, B, R, R, Cc, Cc, s())
    with pytest.raises(RuntimeError, match="flowedit_step: bad shape"):
        _lib.call("fluxmi_flowedit_step", *args(c_in=60, c_out=60))
    prog3 = flowedit.build_program(ts, 3)
    _, ctl3 = tables(prog3, dev)
    steps = [torch.tensor([j], dtype=torch.int32, device=dev) for j in (0, 1, 2)]
    for st in steps:  # first without apply, neither, apply without first: each needs the accumulator
        with pytest.raises(RuntimeError, match="NULL acc"):
            _lib.call("fluxmi_flowedit_step", *args(ctl=ctl3, step=ops._p(st)))
    torch.cuda.synchronize()
    assert torch.equal(zz, want_z) and torch.equal(img, want_img), "a refused call wrote"


# ---- engine helpers -----------------------------------------------------------------------------------------------------------------------
def run_edit(model, d, ts, z=None, x0=None, n_avg=1, ids=None, off=0, gs=GS, gt=GT, use_graph=True, swap=False, **kw):
    """the source branch is the helpers' negative prompt, the target branch their prompt; x0 their noise tensor"""
    B = d["img"].shape[0]
    src, tar = ("txt", "y"), ("neg_txt", "neg_y")
    if not swap:
        src, tar = tar, src
    x0 = d["img"] if x0 is None else x0
    return model.denoise_edit(x0 if z is None else z, d["img_ids"], d[src[0]], d[src[1]], d[tar[0]], d[tar[1]], d["txt_ids"], ts, n_avg=n_avg,
                              ids=IDS3[:B] if ids is None else ids, eval_offset=off, source_guidance=gs, guidance=gt, use_graph=use_graph, x0=x0, **kw)


def python_edit_loop(model, d, ts, z, x0, n_avg, ids, off, mode, gs=GS, gt=GT):
    """model(...) per evaluation on the 2B batch with the per-sample guidance vector, and the C-entry kernels"""
    from fluxmi import flowedit, ops

    dev, B = z.device, z.shape[0]
    prog = flowedit.build_program(ts, n_avg)
    coef, ctl = tables(prog, dev)
    g = torch.tensor([gs] * B + [gt] * B, dtype=torch.bfloat16, device=dev)
    txt, y = torch.cat((d["neg_txt"], d["txt"]), 0), torch.cat((d["neg_y"], d["y"]), 0)
    acc = torch.zeros(z.shape, dtype=torch.float32, device=dev) if flowedit.needs_acc(prog) else None
    z = z.clone()
    img = ops.flowedit_couple(z, x0, prog.times[0], ids, off)
    step, offt = torch.zeros(1, dtype=torch.int32, device=dev), torch.tensor([off], dtype=torch.int32, device=dev)
    for j, t in enumerate(prog.times):
        tv = torch.full((2 * B,), t, dtype=torch.bfloat16, device=dev)
        pred = model(img, dup(d["img_ids"]), txt, dup(d["txt_ids"]), tv, y, g, mode=mode).contiguous()
        step.fill_(j)
        ops.flowedit_step(img, pred, z, x0, coef, ctl, ids, acc=acc, step=step, eval_offset=offt)
    return z


def captures(model):
    from fluxmi import _lib

    c, r = C.c_longlong(0), C.c_int(0)
    _lib.call("fluxmi_engine_preview_stats", model._engine, C.byref(c), C.byref(r))
    return c.value


# ---- 2. engine: graph == eager == python loop; tuning knobs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_edit_denoise_bit_exact(dev, qname):
    from fluxmi import _lib

    cfg = tiny_config()
    model, _ = build(cfg, QUANTS[qname], dev)
    B = 2
    d = to_dev(inputs("plain", cfg.params, 64, 64, 32, B, seed=5), dev)
    x0 = d["img"]
    x0_kept = x0.clone()
    ts = fo.get_schedule(16, x0.shape[1])
    lat = run_edit(model, d, ts[:14], use_graph=False)  # fp8: 13 calibrating edit evaluations (one trial each), then frozen
    assert lat.shape == x0.shape and lat.dtype == torch.bfloat16 and torch.isfinite(lat).all()
    if qname == "fp8":
        assert model.calibration_state()[0]
    mode = 1 if qname == "fp8" else 2
    ts2 = ts[3:12]
    a = run_edit(model, d, ts2, z=lat, off=13)
    b = run_edit(model, d, ts2, z=lat, off=13, use_graph=False)
    assert torch.equal(a, b), f"graph vs eager: rel-L2 {rel_l2(a, b):.3e}"
    c = python_edit_loop(model, d, ts2, lat, x0, 1, IDS3[:B], 13, mode)
    assert torch.equal(a, c), f"graph loop vs python loop: rel-L2 {rel_l2(a, c):.3e}"
    # averaging: rows without first / apply, the fp32 accumulator in memory
    ts3 = ts[3:7]
    a3 = run_edit(model, d, ts3, z=lat, n_avg=3)
    assert torch.equal(a3, run_edit(model, d, ts3, z=lat, n_avg=3, use_graph=False))
    c3 = python_edit_loop(model, d, ts3, lat, x0, 3, IDS3[:B], 0, mode)
    assert torch.equal(a3, c3), f"n_avg 3, graph loop vs python loop: rel-L2 {rel_l2(a3, c3):.3e}"
    assert torch.equal(a, run_edit(model, d, ts2, z=lat, off=13)), "the averaging request left something behind"
    fresh = run_edit(model, d, ts2)  # from x0
    assert not torch.equal(fresh, x0), "the edit moved nothing"
    assert not torch.equal(fresh, run_edit(model, d, ts2, swap=True)), "source and target swapped give the same bits"
    assert torch.equal(x0, x0_kept) and torch.equal(d["img"], x0_kept), "the caller's x0 changed"
    if qname == "fp8":
        for knobs in KNOB_SETS:
            with _lib.tuning(**knobs):
                ak = run_edit(model, d, ts2, z=lat, off=13)
            assert torch.equal(a, ak), f"edit latents change under tuning {knobs}: rel-L2 {rel_l2(ak, a):.3e}"


# ---- 3. the graph is keyed on the kind ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_plain_guided_and_edit_requests_never_share_a_graph(dev, qname):
    cfg = tiny_config()
    model, _ = build(cfg, QUANTS[qname], dev)
    d2 = to_dev(inputs("plain", cfg.params, 64, 64, 32, 2, seed=5), dev)
    d1 = {k: v[:1] for k, v in d2.items()}
    ts = fo.get_schedule(16, d2["img"].shape[1])
    lat = plain_denoise(model, d2, ts[:14], use_graph=False)
    ts2 = ts[:7]
    # one prepared shape (two samples): plain B = 2, guided B = 1, edit B = 1, in turn
    runs = [lambda: plain_denoise(model, d2, ts2, img=lat), lambda: guided_denoise(model, d1, ts2, img=lat[:1]),
            lambda: run_edit(model, d1, ts2, x0=lat[:1])]
    first = [r() for r in runs]
    assert not torch.equal(first[1], first[2])
    for _ in range(2):
        for i, r in enumerate(runs):
            again = r()
            assert torch.equal(first[i], again), f"request kind {i} differs from its own first result: rel-L2 {rel_l2(again, first[i]):.3e}"


# ---- 4. draws and slices ------------------------------------------------------------------------------------------------------------------
def test_draws_and_slices(dev):
    from fluxmi import flowedit

    cfg = tiny_config()
    model, _ = build(cfg, QUANTS["fp8"], dev)
    d2 = to_dev(inputs("plain", cfg.params, 64, 64, 32, 2, seed=9), dev)
    d1 = {k: v[:1] for k, v in d2.items()}
    ts = fo.get_schedule(16, d2["img"].shape[1])
    run_edit(model, d1, ts[:14], use_graph=False)
    assert model.calibration_state()[0]
    ts2, k = ts[2:11], 3  # n = 8 evaluations
    ids = flowedit.edit_ids(77, 2)
    whole = run_edit(model, d1, ts2, ids=ids[:1])
    head = run_edit(model, d1, ts2[:k + 1], ids=ids[:1])
    tail = run_edit(model, d1, ts2[k:], z=head, ids=ids[:1], off=k)
    assert torch.equal(whole, tail), f"k + (n - k) evaluations differ from n: rel-L2 {rel_l2(tail, whole):.3e}"
    assert not torch.equal(tail, run_edit(model, d1, ts2[k:], z=head, ids=ids[:1], off=0)), "the offset has no effect"
    # another seed: other bits, the same graph
    run_edit(model, d1, ts2, ids=ids[:1])
    c0 = captures(model)
    other = run_edit(model, d1, ts2, ids=flowedit.edit_ids(78, 1))
    assert captures(model) == c0, "a new seed re-captured the step graph"
    assert not torch.equal(other, whole)
    # image 1 of a two-image request == the same image alone under its own ids
    both = run_edit(model, d2, ts2, ids=ids)
    one = run_edit(model, {k_: v[1:2] for k_, v in d2.items()}, ts2, ids=ids[1:2])
    assert torch.equal(one[0], both[1]), f"a sample depends on its batch: rel-L2 {rel_l2(one[0], both[1]):.3e}"
    assert torch.equal(whole[0], both[0])


# ---- 5. a guidance value per branch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schnell", [False, True], ids=["dev", "schnell"])
def test_per_branch_guidance_reaches_the_model(dev, schnell):
    cfg = tiny_config(schnell=schnell)
    model, _ = build(cfg, QUANTS["bf16"], dev)
    d = to_dev(inputs("plain", cfg.params, 64, 64, 32, 1, seed=3), dev)
    ts = fo.get_schedule(8, d["img"].shape[1], shift=not schnell)[:5]
    same = run_edit(model, d, ts, gs=GT, gt=GT)
    split = run_edit(model, d, ts, gs=GS, gt=GT)
    flipped = run_edit(model, d, ts, gs=GT, gt=GS)
    if schnell:  # no guidance embedder: both values are ignored
        assert torch.equal(same, split) and torch.equal(same, flipped)
    else:
        assert not torch.equal(same, split), "source_guidance does not reach the source branch"
        assert not torch.equal(same, flipped), "guidance does not reach the target branch"
        assert not torch.equal(split, flipped)


# ---- 6. against the oracle ------------------------------------------------------------------------------------------------------------------
def oracle_edit_loop(oracle, inp, ts, draws, gs=GS, gt=GT):
    """FluxOracle.forward on the 2B batch with the per-sample guidance vector + flowedit_ref's bf16 chain on the normals read back from the GPU"""
    from fluxmi import flowedit

    x0 = inp["img"].to(torch.bfloat16)
    B = x0.shape[0]
    prog = flowedit.build_program(ts, 1)
    g = torch.tensor([gs] * B + [gt] * B, dtype=oracle.dtype)
    txt, y = torch.cat((inp["neg_txt"], inp["txt"]), 0), torch.cat((inp["neg_y"], inp["y"]), 0)
    z = x0.clone()
    img = torch.cat(fr.couple_bf16(z, x0, prog.times[0], 1.0 - prog.times[0], draws[0]), 0)
    for j, t in enumerate(prog.times):
        tv = torch.full((2 * B,), t, dtype=oracle.dtype)
        pred = oracle.forward(img, dup(inp["img_ids"]), txt, dup(inp["txt_ids"]), tv, y, g).to(torch.bfloat16)
        img, z, _ = fr.step_bf16(pred, z, None, x0, prog.coef[j], prog.ctl[j], draws[j + 1])
    return z


@pytest.mark.parametrize("schnell", [False, True], ids=["dev", "schnell"])
def test_edit_denoise_matches_oracle(dev, schnell, monkeypatch):
    """B = 1, 64 x 64, Lt 32, 16 evaluations (n_avg 1) through calibration, guidance 1.5 / 5.5.  The gates are those of
    test_cfg_gpu.test_guided_denoise_matches_oracle, on the result z:
      fp8 flows: rel-L2(engine, oracle-bf16) <= 1.25 x rel-L2(oracle-fp8, oracle-bf16);
      bf16 flow: rel-L2(engine, oracle-bf16) <= max(1e-2, 1.75 x floor), floor = the bf16 oracle's own movement under fo.attention_exact.
    Printed without a gate: the same three distances on the displacement z - x0 (profiles/flowedit.txt records a run)."""
    H, W, Lt, B, n = 64, 64, 32, 1, 16
    ts = fo.get_schedule(n, (H // 16) * (W // 16), shift=not schnell)
    tag = "schnell" if schnell else "dev"
    ids = IDS3[:B]
    ref = {}
    for qname in QUANTS:
        cfg = tiny_config(schnell=schnell)
        model, sd = build(cfg, QUANTS[qname], dev)
        inp = inputs("plain", cfg.params, H, W, Lt, B, seed=7)
        x0 = inp["img"].float()
        disp = lambda a, b: rel_l2(a.float().cpu() - x0, b.float().cpu() - x0)
        if not ref:
            ref["draws"] = [normals(dev, ids, tuple(inp["img"].shape[1:]), k).cpu() for k in range(n + 1)]
            ref["o16"] = oracle_edit_loop(make_oracle(cfg, sd, None), inp, ts, ref["draws"])
            with monkeypatch.context() as mp:
                mp.setattr(fo, "attention", fo.attention_exact)
                ref["o16x"] = oracle_edit_loop(make_oracle(cfg, sd, None), inp, ts, ref["draws"])
            ref["floor16"] = rel_l2(ref["o16x"], ref["o16"])
        got = run_edit(model, to_dev(inp, dev), ts, ids=ids)
        assert got.shape == inp["img"].shape and torch.isfinite(got).all()
        e16 = rel_l2(got, ref["o16"])
        if qname == "bf16":
            gate = max(1e-2, 1.75 * ref["floor16"])
            print(f"[flowedit {tag} bf16] engine vs oracle-bf16 {e16:.3e}; floor (oracle-bf16, exact attention) {ref['floor16']:.3e}; gate {gate:.3e}; "
                  f"on z - x0: engine {disp(got, ref['o16']):.3e}, floor {disp(ref['o16x'], ref['o16']):.3e}")
            assert e16 <= gate, f"{tag} bf16: rel-L2 {e16:.3e} > max(1e-2, 1.75 x {ref['floor16']:.3e})"
        else:
            o8 = oracle_edit_loop(make_oracle(cfg, sd, QUANTS[qname]), inp, ts, ref["draws"])
            yard = rel_l2(o8, ref["o16"])
            print(f"[flowedit {tag} {qname}] engine vs oracle-bf16 {e16:.3e}; yardstick (oracle-fp8 vs oracle-bf16) {yard:.3e}; ratio "
                  f"{e16 / yard:.3f} (gate 1.25); engine vs oracle-fp8 {rel_l2(got, o8):.3e}; on z - x0: engine {disp(got, ref['o16']):.3e}, "
                  f"yardstick {disp(o8, ref['o16']):.3e}, engine vs oracle-fp8 {disp(got, o8):.3e}")
            assert e16 <= 1.25 * yard, f"{tag} {qname}: vs bf16 flow {e16:.3e} > 1.25 x {yard:.3e}"


# ---- 7. pipeline --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe(dev):
    p = tiny_pipeline(dev)
    p.compile()
    assert p.model.calibration_state()[0]
    return p


def test_pipeline_flow_edit(dev, pipe):
    import numpy as np
    from PIL import Image

    from fluxmi import GenerationCancelled, flowedit, ops

    tar, src = prompts()
    photo = np.random.default_rng(0).integers(0, 256, size=(96, 64, 3), dtype=np.uint8)
    H, W, n = 96, 64, 6
    kw = dict(init_image=photo, source_prompt=src, width=W, height=H, num_steps=n, seed=7, silent=True, source_guidance=GS, guidance=GT)
    plain_kw = dict(width=W, height=H, num_steps=n, seed=7, silent=True, output_type="latent")
    plain_before = pipe.generate(tar, **plain_kw)
    a = pipe.generate(tar, output_type="latent", **kw)
    assert torch.equal(a, pipe.generate(tar, output_type="latent", **kw)), "same seed, different latents"
    assert torch.isfinite(a).all() and not torch.equal(a, plain_before)
    # == Flux.denoise_edit on prepare's tensors
    latent, ts = pipe.prepare_edit(pipe.load_init_image_if_needed(photo), H, W, n, 1)
    assert len(ts) == n + 1 and not torch.equal(a.cpu(), latent.float().cpu()), "the edit moved nothing"
    x0, img_ids, vec, txt, txt_ids = map(lambda t: t.contiguous(), pipe.prepare(latent, tar))
    _, _, svec, stxt, _ = pipe.prepare(latent, src)
    ids = flowedit.edit_ids(7, 1)
    ed = lambda tsl, **k: pipe.model.denoise_edit(x0, img_ids, stxt, svec, txt, vec, txt_ids, tsl, ids=ids, source_guidance=GS, guidance=GT, **k)
    assert torch.equal(a, pipe.unpack(ed(ts).float(), H, W))
    # noise_seed replaces the request's seed as the key; source_guidance = None means guidance
    assert torch.equal(pipe.generate(tar, output_type="latent", **{**kw, "seed": 3, "noise_seed": 7}), a)
    assert not torch.equal(pipe.generate(tar, output_type="latent", **{**kw, "noise_seed": 8}), a)
    same_g = pipe.model.denoise_edit(x0, img_ids, stxt, svec, txt, vec, txt_ids, ts, ids=ids, source_guidance=GT, guidance=GT)
    assert torch.equal(pipe.generate(tar, output_type="latent", **{**kw, "source_guidance": None}), pipe.unpack(same_g.float(), H, W))
    # n_max < num_steps: the sliced schedule
    assert torch.equal(pipe.generate(tar, output_type="latent", edit_n_max=4, **kw), pipe.unpack(ed(ts[2:]).float(), H, W))
    assert torch.equal(pipe.generate(tar, output_type="latent", edit_n_max=0, **kw), pipe.unpack(x0.float(), H, W))
    # n_min = 2: coupled steps, one more coupling, plain denoise on the target prompt
    z = ed(ts[:n - 1], n_avg=2)
    zt = ops.flowedit_couple(z, x0.to(torch.bfloat16).contiguous(), ts[n - 2], ids, 2 * (n - 2))[1:]
    want = pipe.model.denoise(zt, img_ids, txt, txt_ids, vec, ts[n - 2:], guidance=GT)
    got = pipe.generate(tar, output_type="latent", edit_n_min=2, edit_n_avg=2, **kw)
    assert torch.equal(got, pipe.unpack(want.float(), H, W)) and not torch.equal(got, a)
    # num_images = 2: the same photo and prompts, different draws
    two = pipe.generate(tar, output_type="latent", num_images=2, **kw)
    assert two.shape[0] == 2 and torch.equal(two[0], a[0]) and not torch.equal(two[0], two[1])
    # through the VAE
    px = torch.as_tensor(pipe.generate(tar, output_type="uint8", **kw))
    assert px.dtype == torch.uint8 and tuple(px.shape) == (1, H, W, 3) and px.float().std() > 0
    buf = pipe.generate(tar, **kw)
    assert isinstance(buf, io.BytesIO) and Image.open(buf).size == (W, H)
    # on_step: once per evaluation (coupled steps x n_avg, then the tail), numbered through; False cancels
    seen = []
    out = pipe.generate(tar, output_type="latent", edit_n_min=2, edit_n_avg=2, on_step=lambda info: seen.append(info) or True, **kw)
    assert torch.equal(out, got)
    assert [i["evaluation"] for i in seen] == list(range(2 * (n - 2) + 2)) and all(i["num_evaluations"] == 2 * (n - 2) + 2 for i in seen)
    assert [i["step"] for i in seen] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 5] and all(i["preview"] is None for i in seen)
    with pytest.raises(GenerationCancelled):
        pipe.generate(tar, output_type="latent", on_step=lambda info: info["evaluation"] < 1, **kw)
    # the engine is as usable as before: the edit again, and a plain request equal to the one before any edit
    assert torch.equal(pipe.generate(tar, output_type="latent", **kw), a)
    assert torch.equal(pipe.generate(tar, **plain_kw), plain_before)
    with pytest.raises(ValueError, match="sequence length"):
        pipe.generate(tar, output_type="latent", **{**kw, "source_prompt": {"txt": src["txt"][:, :16], "vec": src["vec"]}})


# ---- 8. real width -----------------------------------------------------------------------------------------------------------------------
def test_edit_at_1024_real_width(dev):
    """hidden 3072, 1 + 1 blocks, 1024^2, Lt 512, one image (two samples in the engine), 3 evaluations on a frozen model: graph == eager, finite"""
    import util

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    cfg.params.depth, cfg.params.depth_single_blocks = 1, 1
    model, _ = build(cfg, QUANTS["fp8"], dev, seed=2)
    d = to_dev(inputs("plain", cfg.params, 1024, 1024, 512, 1, seed=8, real_tokens=64), dev)
    Li = d["img"].shape[1]
    assert Li + 512 == 4608
    ts = fo.get_schedule(16, Li)
    lat = run_edit(model, d, ts[:14], use_graph=False)  # calibrate at this shape
    assert model.calibration_state()[0] and torch.isfinite(lat).all()
    ts2 = ts[4:8]
    a = run_edit(model, d, ts2, z=lat, off=13)
    b = run_edit(model, d, ts2, z=lat, off=13, use_graph=False)
    assert torch.isfinite(a).all() and torch.equal(a, b), f"graph vs eager: rel-L2 {rel_l2(a, b):.3e}"
    assert not torch.equal(a, lat)
    print(f"[flowedit 1024^2 B=1] graph == eager; z std {a.float().std().item():.3f}")
