"""Negative prompts (true classifier-free guidance) on the GPU.  The image stream of a guided request holds 2B samples, the prompt branches
first and the negative branches of the same images behind them; every step is one forward on the 2B samples and the guided Euler update

    x' = x + (t_prev - t_curr) * (u + s * (c - u))          c = pred[:B], u = pred[B:], every operation rounded to bf16 once,

written to both halves (csrc/update_step.hip, the guided arm of euler_kernel).  The oracle needs no change: a guided step is FluxOracle.forward on the 2B
batch followed by that torch expression.  Helpers are those of tests/test_fill_gpu.py / tests/test_kontext_gpu.py, copied."""
import ctypes as C
import io
import math

import pytest
import torch

import flux_oracle as fo

pytestmark = pytest.mark.gpu

SCALE = 3.5
IN_CHANNELS = {"plain": 64, "kontext": 64, "fill": 384}


def tiny_config(kind="plain", schnell=False):
    import util

    cfg = util.load_config(util.ModelVersion.flux_schnell if schnell else util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    p = cfg.params
    p.hidden_size, p.num_heads, p.depth, p.depth_single_blocks, p.context_in_dim, p.vec_in_dim = 256, 2, 2, 2, 128, 64
    if IN_CHANNELS[kind] != 64:
        p.in_channels, p.out_channels = IN_CHANNELS[kind], 64
    return cfg


def state_dict(params, seed):
    """tests/test_engine_gpu.py's text-to-image test model; for a channel-conditioned model the same weights plus img_in columns for the
    conditioning channels (tests/test_fill_gpu.py, conditioned_state_dict)"""
    from fluxmi import synth

    if params.in_channels == 64:
        return synth.make_state_dict(params, seed=seed)
    plain = params.model_copy(update={"in_channels": 64, "out_channels": None})
    sd = synth.make_state_dict(plain, seed=seed)
    K = params.in_channels
    g = torch.Generator().manual_seed(700 + seed)
    extra = (torch.rand(params.hidden_size, K - 64, generator=g) * 2 - 1) * math.sqrt(3.0 / K)
    sd["img_in.weight"] = torch.cat((sd["img_in.weight"].float(), extra), 1).to(sd["img_in.weight"].dtype)
    return sd


def build(cfg, quant, dev, seed=0):
    import util
    from float8_quantize import quantize_flow_transformer_and_dispatch_float8

    sd = state_dict(cfg.params, seed)
    model = util.load_flow_model(cfg, {k: v.clone() for k, v in sd.items()})
    model.to(dev)
    if quant is not None:
        quantize_flow_transformer_and_dispatch_float8(model, dev, flow_dtype=torch.bfloat16, swap_linears_with_cublaslinear=False,
                                                      quantize_modulation=quant["modulation"], quantize_flow_embedder_layers=quant["embedders"])
    return model, sd


def make_oracle(cfg, sd, quant):
    return fo.FluxOracle({k: v.clone() for k, v in sd.items()}, fo.FluxParams(**cfg.params.model_dump()), quantize=quant)


def rel_l2(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def to_dev(inp, dev):
    return {k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in inp.items()}


QUANTS = {
    "bf16": None,
    "fp8": dict(modulation=True, embedders=False),
    "fp8_emb": dict(modulation=True, embedders=True),
}


def inputs(kind, params, H, W, Lt, B, seed, real_tokens=8):
    """synth.make_inputs for the prompt branch, the negative branch's txt / y from make_inputs with another seed, and the stream's
    conditioning: Kontext reference tokens on a 3 x 3 grid (`seq`, `seq_ids`) or Fill's 320 conditioning channels (`cond`)"""
    from flux_pipeline import FluxPipeline, kontext_reference_ids
    from fluxmi import synth

    inp = synth.make_inputs(params, H, W, Lt, batch=B, seed=seed, real_tokens=real_tokens)
    neg = synth.make_inputs(params, H, W, Lt, batch=B, seed=seed + 100, real_tokens=real_tokens // 2)
    inp["neg_txt"], inp["neg_y"] = neg["txt"], neg["y"]
    g = torch.Generator().manual_seed(500 + seed)
    Li = inp["img"].shape[1]
    if kind == "kontext":
        inp["seq"] = torch.randn(B, 9, params.in_channels, generator=g).to(torch.bfloat16)
        inp["seq_ids"] = kontext_reference_ids(B, 6, 6, "cpu", torch.bfloat16)
    if kind == "fill":
        cond = torch.randn(B, Li, 64, generator=g).to(torch.bfloat16)
        m = torch.zeros(B, 1, H, W)
        for b in range(B):
            y0, x0 = int(torch.randint(0, H // 2, (1,), generator=g)), int(torch.randint(0, W // 2, (1,), generator=g))
            m[b, :, y0:y0 + H // 2 + 3, x0:x0 + W // 3 + 5] = 1.0
        inp["cond"] = torch.cat((cond, FluxPipeline.pack_fill_mask(m)), -1)
    return inp


def cond_kw(d):
    kw = {}
    if "seq" in d:
        kw.update(img_cond_seq=d["seq"], img_cond_seq_ids=d["seq_ids"])
    if "cond" in d:
        kw.update(img_cond=d["cond"])
    return kw


def plain_denoise(model, d, ts, use_graph=True, img=None):
    return model.denoise(d["img"] if img is None else img, d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts, guidance=3.5, use_graph=use_graph,
                         **cond_kw(d))


def guided_denoise(model, d, ts, use_graph=True, img=None, scale=SCALE):
    return model.denoise(d["img"] if img is None else img, d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts, guidance=3.5, use_graph=use_graph,
                         neg_txt=d["neg_txt"], neg_y=d["neg_y"], cfg_scale=scale, **cond_kw(d))


def dup(t):
    return torch.cat((t, t), 0)


def python_guided_loop(model, d, ts, x, mode, scale=SCALE):
    """model(cat(x, x), ..., cat(txt, neg_txt), ...) per step and the torch expression of the guided update"""
    B = x.shape[0]
    g = torch.full((2 * B,), 3.5, dtype=torch.bfloat16, device=x.device)
    kw = {k: dup(v) for k, v in cond_kw(d).items()}
    txt, y = torch.cat((d["txt"], d["neg_txt"]), 0), torch.cat((d["y"], d["neg_y"]), 0)
    for t_curr, t_prev in zip(ts[:-1], ts[1:]):
        tv = torch.full((2 * B,), t_curr, dtype=torch.bfloat16, device=x.device)
        pred = model(dup(x), dup(d["img_ids"]), txt, dup(d["txt_ids"]), tv, y, g, mode=mode, **kw)
        c, u = pred[:B], pred[B:]
        x = x + (t_prev - t_curr) * (u + scale * (c - u))
    return x


def oracle_guided_loop(oracle, inp, ts, scale=SCALE, guidance=3.5):
    """fo.denoise with both branches in one FluxOracle.forward on the 2B batch and the guided update (bf16 tensors, python scalars)"""
    x = inp["img"]
    B = x.shape[0]
    g = torch.full((2 * B,), guidance, dtype=oracle.dtype)
    txt, y = torch.cat((inp["txt"], inp["neg_txt"]), 0), torch.cat((inp["y"], inp["neg_y"]), 0)
    for t_curr, t_prev in zip(ts[:-1], ts[1:]):
        tv = torch.full((2 * B,), t_curr, dtype=oracle.dtype)
        pred = oracle.forward(dup(x), dup(inp["img_ids"]), txt, dup(inp["txt_ids"]), tv, y, g)
        c, u = pred[:B], pred[B:]
        x = x + (t_prev - t_curr) * (u + scale * (c - u))
    return x


# ---- 1. the kernel against the torch expression -------------------------------------------------------------------------------------
LAYOUTS = {"plain": (15, 15, 64, 64), "rows": (15 + 9, 15, 64, 64), "cols": (15, 15, 384, 64)}  # img_rows, pred_rows (odd), c_in, c_out


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("B", [1, 3])
def test_cfg_euler_kernel_bit_exact(dev, layout, B):
    from fluxmi import _lib, ops

    R, Rp, Ci, Co = LAYOUTS[layout]
    g = torch.Generator().manual_seed(11 + B)
    dts = torch.tensor([-0.0625, -0.03173828125, 0.0471], dtype=torch.float32)
    for scale in (0.0, 1.0, 3.5, 7.25):
        for step in (0, 2):
            # the two halves of the stream start DIFFERENT: the kernel must read x from the prompt half alone and write both
            img = torch.randn(2 * B, R, Ci, generator=g).to(torch.bfloat16).to(dev)
            pred = torch.randn(2 * B, Rp, Co, generator=g).to(torch.bfloat16).to(dev)
            before = img.clone()
            c, u, x = pred[:B], pred[B:], img[:B, :Rp, :Co]
            want = x + float(dts[step]) * (u + scale * (c - u))
            assert want.dtype == torch.bfloat16
            d_dts, d_step, d_scale = dts.to(dev), torch.tensor([step], dtype=torch.int32, device=dev), torch.tensor([scale], dtype=torch.float32, device=dev)
            _lib.call("fluxmi_cfg_euler", ops._p(img), ops._p(pred), ops._p(d_dts), ops._p(d_step), ops._p(d_scale), B, R, Rp, Ci, Co, ops._stream())
            torch.cuda.synchronize()
            assert torch.equal(img[:B, :Rp, :Co], want), f"{layout} B={B} s={scale} step={step}: rel-L2 {rel_l2(img[:B, :Rp, :Co], want):.3e}"
            assert torch.equal(img[B:, :Rp, :Co], img[:B, :Rp, :Co]), "the halves differ after the update"
            assert torch.equal(img[:, Rp:], before[:, Rp:]), "reference rows changed"
            assert torch.equal(img[..., Co:], before[..., Co:]), "conditioning channels changed"
    # step = NULL reads dts[0], like fluxmi_euler
    img = torch.randn(2 * B, R, Ci, generator=g).to(torch.bfloat16).to(dev)
    want = img[:B, :Rp, :Co] + float(dts[0]) * (pred[B:] + 2.0 * (pred[:B] - pred[B:]))
    d_scale = torch.tensor([2.0], dtype=torch.float32, device=dev)
    _lib.call("fluxmi_cfg_euler", ops._p(img), ops._p(pred), ops._p(d_dts), None, ops._p(d_scale), B, R, Rp, Ci, Co, ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(img[:B, :Rp, :Co], want)
    with pytest.raises(RuntimeError, match="cfg_euler: bad shape"):
        _lib.call("fluxmi_cfg_euler", ops._p(img), ops._p(pred), ops._p(d_dts), None, ops._p(d_scale), B, Rp, R + 1, Ci, Co, ops._stream())


@pytest.mark.parametrize("guided", [False, True])
def test_euler_kernel_second_grid_trip(dev, guided):
    """The grid is capped at 4096 workgroups of 256 threads = 1 048 576 vectors; 131073 rows of 64 channels are 1 048 584, so eight threads
    take the grid-stride loop's second trip.  fluxmi_euler and the plain fluxmi_cfg_euler (B = 1) against the torch bf16 expression, bit for
    bit, with a NaN-pattern guard region behind the stream that must come back untouched."""
    from fluxmi import _lib, ops

    R, C, GUARD, halves = 131073, 64, 4096, 2 if guided else 1
    g = torch.Generator().manual_seed(29)
    n = halves * R * C
    store = torch.full((n + GUARD,), 0x7FC1, dtype=torch.int16).view(torch.bfloat16).to(dev)  # a quiet NaN with a payload no kernel writes
    guard_before = store[n:].view(torch.int16).clone()
    store[:n] = torch.randn(n, generator=g).to(torch.bfloat16).to(dev)
    img = store[:n].view(halves, R, C)
    pred = torch.randn(halves, R, C, generator=g).to(torch.bfloat16).to(dev)
    dts = torch.tensor([0.0471, -0.03173828125], dtype=torch.float32)
    d_dts, d_step = dts.to(dev), torch.tensor([1], dtype=torch.int32, device=dev)
    if guided:
        c, u = pred[:1], pred[1:]
        want = img[:1] + float(dts[1]) * (u + SCALE * (c - u))
        d_scale = torch.tensor([SCALE], dtype=torch.float32, device=dev)
        _lib.call("fluxmi_cfg_euler", ops._p(img), ops._p(pred), ops._p(d_dts), ops._p(d_step), ops._p(d_scale), 1, R, R, C, C, ops._stream())
    else:
        want = img + float(dts[1]) * pred
        _lib.call("fluxmi_euler", ops._p(img), ops._p(pred), ops._p(d_dts), ops._p(d_step), R * C, ops._stream())
    torch.cuda.synchronize()
    assert want.dtype == torch.bfloat16
    for h in range(halves):
        assert torch.equal(img[h], want[0]), f"half {h}: {(img[h] != want[0]).sum().item()} elements differ, {(img[h, -1] != want[0, -1]).sum().item()} in the last row"
    assert torch.equal(store[n:].view(torch.int16), guard_before), "the guard region behind the stream changed"


# ---- 2. guided denoise: graph == eager == python loop; 7. tuning knobs ----------------------------------------------------------------------
KNOB_SETS = (dict(prefetch=0), dict(prefetch=2), dict(gemm_persist=0), dict(qlut=0), dict(fuse_kv=1), dict(fuse_kv=0), dict(w_pairs=0), dict(a_pairs=0))


@pytest.mark.parametrize("kind", list(IN_CHANNELS))
@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_guided_denoise_bit_exact(dev, qname, kind):
    from fluxmi import _lib

    cfg = tiny_config(kind)
    model, _ = build(cfg, QUANTS[qname], dev)
    B, H, W, Lt = 2, 64, 64, 32
    d = to_dev(inputs(kind, cfg.params, H, W, Lt, B, seed=5), dev)
    kept = {k: d[k].clone() for k in ("seq", "cond") if k in d}
    ts = fo.get_schedule(16, d["img"].shape[1])
    lat = guided_denoise(model, d, ts[:14], use_graph=False)  # fp8: 13 calibrating GUIDED steps (one trial per step), then frozen
    assert lat.shape == d["img"].shape and torch.isfinite(lat).all()
    if qname == "fp8":
        assert model.calibration_state()[0]
    ts2 = ts[:9]
    a = guided_denoise(model, d, ts2, img=lat)
    b = guided_denoise(model, d, ts2, img=lat, use_graph=False)
    assert a.shape == d["img"].shape and a.dtype == torch.bfloat16
    assert torch.equal(a, b), f"graph vs eager: rel-L2 {rel_l2(a, b):.3e}"
    c = python_guided_loop(model, d, ts2, lat.clone(), mode=1 if qname == "fp8" else 2)
    assert torch.equal(a, c), f"graph loop vs python loop: rel-L2 {rel_l2(a, c):.3e}"
    assert not torch.equal(a, plain_denoise(model, d, ts2, img=lat)), "the negative branch has no effect"
    for k, v in kept.items():
        assert torch.equal(d[k], v), f"the caller's {k} changed"
    if qname == "fp8":
        for knobs in KNOB_SETS:
            with _lib.tuning(**knobs):
                a3 = guided_denoise(model, d, ts2, img=lat)
            assert torch.equal(a, a3), f"guided latents change under tuning {knobs}: rel-L2 {rel_l2(a3, a):.3e}"


def test_c_entry_steps_the_callers_samples_in_place(dev):
    """fluxmi_engine_denoise_cfg on a caller-owned [B, Li, C_in] stream of a Fill model: the conditioning channels come back bit for bit, the
    noisy channels equal Flux.denoise's"""
    from fluxmi import _lib, ops

    cfg = tiny_config("fill")
    model, _ = build(cfg, None, dev)
    B, Lt = 2, 32
    d = to_dev(inputs("fill", cfg.params, 64, 64, Lt, B, seed=6), dev)
    ts = fo.get_schedule(16, d["img"].shape[1])[:7]
    want = guided_denoise(model, d, ts)
    full = torch.cat((d["img"], d["cond"]), -1).contiguous()
    txt, y = torch.cat((d["txt"], d["neg_txt"]), 0).contiguous(), torch.cat((d["y"], d["neg_y"]), 0).contiguous()
    t_io = C.c_int(0)
    tsc = (C.c_double * len(ts))(*ts)
    with model._lock:  # the engine is still prepared for this request's 2B samples
        _lib.call("fluxmi_engine_denoise_cfg", model._engine, ops._p(full), ops._p(txt), ops._p(y), 3.5, SCALE, tsc, len(ts) - 1, C.byref(t_io), 1,
                  ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(full[..., 64:], d["cond"]) and torch.equal(full[..., :64], want)


# ---- 3. the graph is keyed on guidance --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_plain_and_guided_requests_never_share_a_graph(dev, qname):
    cfg = tiny_config()
    model, _ = build(cfg, QUANTS[qname], dev)
    Lt = 32
    d2 = to_dev(inputs("plain", cfg.params, 64, 64, Lt, 2, seed=5), dev)
    d1 = {k: v[:1] for k, v in d2.items()}
    ts = fo.get_schedule(16, d2["img"].shape[1])
    lat = plain_denoise(model, d2, ts[:14], use_graph=False)
    ts2 = ts[:9]
    # the same prepared shape (2 samples) four times on ONE engine: plain B = 2, guided B = 1, plain B = 2, guided B = 1 at another scale
    runs = [lambda: plain_denoise(model, d2, ts2, img=lat), lambda: guided_denoise(model, d1, ts2, img=lat[:1]),
            lambda: plain_denoise(model, d2, ts2, img=lat), lambda: guided_denoise(model, d1, ts2, img=lat[:1], scale=2.0)]
    got = [r() for r in runs]
    assert not torch.equal(got[1], got[3]), "the scale has no effect"
    for i, r in enumerate(runs):
        model._invalidate_engine()
        fresh = r()
        assert torch.equal(got[i], fresh), f"request {i} on the shared engine differs from a fresh engine: rel-L2 {rel_l2(got[i], fresh):.3e}"


# ---- 4. batch invariance ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_a_guided_sample_does_not_depend_on_its_batch(dev, qname):
    cfg = tiny_config()
    model, _ = build(cfg, QUANTS[qname], dev)
    d = to_dev(inputs("plain", cfg.params, 64, 64, 32, 2, seed=9), dev)  # two different (prompt, negative prompt) pairs
    assert not torch.equal(d["txt"][0], d["txt"][1]) and not torch.equal(d["neg_txt"][0], d["neg_txt"][1])
    ts = fo.get_schedule(16, d["img"].shape[1])
    lat = guided_denoise(model, d, ts[:14], use_graph=False)
    ts2 = ts[:9]
    both = guided_denoise(model, d, ts2, img=lat)
    for b in range(2):
        one = guided_denoise(model, {k: v[b:b + 1] for k, v in d.items()}, ts2, img=lat[b:b + 1])
        assert torch.equal(one[0], both[b]), f"sample {b} depends on its batch: rel-L2 {rel_l2(one[0], both[b]):.3e}"
    # [1, ...] negative embeddings are shared by the batch
    shared = guided_denoise(model, {**d, "neg_txt": d["neg_txt"][:1], "neg_y": d["neg_y"][:1]}, ts2, img=lat)
    assert torch.equal(shared[0], both[0]) and not torch.equal(shared[1], both[1])


# ---- pipeline helpers ------------------------------------------------------------------------------------------------------------------
def tiny_pipeline(dev, kind="plain"):
    from flux_pipeline import FluxPipeline
    from modules.autoencoder import AutoEncoder, AutoEncoderParams

    cfg = tiny_config(kind)
    cfg.text_enc_max_length = 32
    cfg.ae_device = str(dev)
    cfg.ae_params = AutoEncoderParams(resolution=32, in_channels=3, ch=32, out_ch=3, ch_mult=[1, 2, 2, 2], num_res_blocks=1, z_channels=16,
                                      scale_factor=0.3611, shift_factor=0.1159)
    torch.manual_seed(0)
    ae_sd = {k: v.clone() for k, v in AutoEncoder(cfg.ae_params).state_dict().items()}
    return FluxPipeline.load_pipeline_from_config(cfg, state_dict=state_dict(cfg.params, 0), ae_state_dict=ae_sd)


def prompts():
    g = torch.Generator().manual_seed(1)
    pos = {"txt": 0.1 * torch.randn(1, 32, 128, generator=g), "vec": torch.randn(1, 64, generator=g)}
    neg = {"txt": 0.1 * torch.randn(1, 32, 128, generator=g), "vec": torch.randn(1, 64, generator=g)}
    return pos, neg


@pytest.fixture(scope="module")
def pipe(dev):
    p = tiny_pipeline(dev)
    p.compile()
    assert p.model.calibration_state()[0]
    return p


# ---- 5. intervals ------------------------------------------------------------------------------------------------------------------------
def test_true_cfg_interval(dev, pipe):
    pos, neg = prompts()
    kw = dict(width=64, height=96, num_steps=8, seed=7, silent=True, output_type="latent")
    gkw = dict(negative_prompt=neg, true_cfg_scale=SCALE)
    plain = pipe.generate(pos, **kw)
    full = pipe.generate(pos, **gkw, **kw)
    assert not torch.equal(full, plain)
    assert torch.equal(pipe.generate(pos, true_cfg_interval=(0, 1), **gkw, **kw), full)
    assert torch.equal(pipe.generate(pos, true_cfg_interval=(0, 0), **gkw, **kw), plain)
    assert torch.equal(pipe.generate(pos, true_cfg_interval=(0.5, 0.5), **gkw, **kw), plain)
    mid = pipe.generate(pos, true_cfg_interval=(0.25, 0.75), **gkw, **kw)
    generator, _ = pipe.set_seed(7)
    noise, ts = pipe.preprocess_latent(height=96, width=64, num_steps=8, generator=generator, num_images=1)
    assert len(ts) == 9
    img, img_ids, vec, txt, txt_ids = map(lambda x: x.contiguous(), pipe.prepare(noise, pos))
    _, _, nvec, ntxt, _ = pipe.prepare(noise, neg)
    x = pipe.model.denoise(img, img_ids, txt, txt_ids, vec, ts[0:3], guidance=3.5)
    x = pipe.model.denoise(x, img_ids, txt, txt_ids, vec, ts[2:7], guidance=3.5, neg_txt=ntxt, neg_y=nvec, cfg_scale=SCALE)
    x = pipe.model.denoise(x, img_ids, txt, txt_ids, vec, ts[6:9], guidance=3.5)
    assert torch.equal(mid, pipe.unpack(x.float(), 96, 64)), "plain(2) -> guided(4) -> plain(2) differs from true_cfg_interval=(0.25, 0.75)"
    assert not torch.equal(mid, full) and not torch.equal(mid, plain)
    with pytest.raises(ValueError, match="true_cfg_interval"):
        pipe.generate(pos, true_cfg_interval=(0.6, 0.4), **gkw, **kw)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(dev, pipe):
    from fluxmi import _lib, ops

    cfg = tiny_config()
    model, _ = build(cfg, None, dev)
    d = to_dev(inputs("plain", cfg.params, 64, 64, 32, 3, seed=2), dev)
    ts = fo.get_schedule(4, d["img"].shape[1])
    plain_denoise(model, d, ts)  # the engine exists and is prepared for an ODD batch (3)
    t_io, tsc = C.c_int(0), (C.c_double * len(ts))(*ts)
    img = d["img"].clone()
    with model._lock, pytest.raises(RuntimeError, match="must be even"):
        _lib.call("fluxmi_engine_denoise_cfg", model._engine, ops._p(img), ops._p(d["txt"]), ops._p(d["y"]), 3.5, SCALE, tsc, len(ts) - 1,
                  C.byref(t_io), 1, ops._stream())
    assert torch.equal(img, d["img"])
    # 2B over the cap (17 images -> 34 samples): no workspace of that batch can be prepared
    ids, tids = d["img_ids"][:1].repeat(34, 1, 1).contiguous(), d["txt_ids"][:1].repeat(34, 1, 1).contiguous()
    with model._lock, pytest.raises(RuntimeError, match=r"B must be 1\.\.32"):
        _lib.call("fluxmi_engine_prepare", model._engine, 34, ids.shape[1], 32, ops._p(ids), ops._p(tids), ops._stream())
    one = {k: v[:1] for k, v in d.items()}
    with pytest.raises(ValueError, match="sequence length"):
        guided_denoise(model, {**one, "neg_txt": torch.cat((one["neg_txt"], one["neg_txt"][:, :1]), 1)}, ts)
    with pytest.raises(ValueError, match="go together"):
        model.denoise(one["img"], one["img_ids"], one["txt"], one["txt_ids"], one["y"], ts, neg_txt=one["neg_txt"])
    with pytest.raises(ValueError, match="go together"):
        model.denoise(one["img"], one["img_ids"], one["txt"], one["txt_ids"], one["y"], ts, neg_y=one["neg_y"])
    with pytest.raises(ValueError, match="neg_y"):
        guided_denoise(model, {**d, "neg_y": d["neg_y"][:2]}, ts)
    pos, neg = prompts()
    with pytest.raises(ValueError, match="needs a negative_prompt"):
        pipe.generate(pos, width=64, height=64, num_steps=4, seed=1, silent=True, true_cfg_scale=2.0)
    with pytest.raises(ValueError, match="sequence length"):
        pipe.generate(pos, width=64, height=64, num_steps=4, seed=1, silent=True, true_cfg_scale=2.0,
                      negative_prompt={"txt": neg["txt"][:, :16], "vec": neg["vec"]})
    # more than 16 images run as equal passes that never split a pair: 18 = 9 + 9, each sample equal to its own guided B = 1 run
    model8, _ = build(cfg, None, dev)
    big = to_dev(inputs("plain", cfg.params, 64, 64, 32, 18, seed=4), dev)
    out = guided_denoise(model8, big, ts)
    assert out.shape == big["img"].shape
    for b in (0, 8, 9, 17):
        assert torch.equal(guided_denoise(model8, {k: v[b:b + 1] for k, v in big.items()}, ts)[0], out[b])


# ---- against the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schnell", [False, True], ids=["dev", "schnell"])
def test_guided_denoise_matches_oracle(dev, schnell, monkeypatch):
    """B = 1, 64 x 64, Lt 32, 16 guided steps through calibration, scale 3.5; the oracle loop is FluxOracle.forward on the 2B batch + the torch
    expression.
    fp8 flows: rel-L2(engine, oracle-bf16 loop) <= 1.25 x rel-L2(oracle-fp8 loop, oracle-bf16 loop) -- gate (iv) with the project's factor.
    bf16 flow: rel-L2(engine, oracle-bf16) <= max(1e-2, 1.75 x floor), floor = the oracle's own movement over the whole guided loop when
    its SDPA is replaced by fo.attention_exact (the form and factor of block_tolerance in tests/test_full_geometry_gpu.py).
    Printed without a gate: the same floor of the fp8 oracle next to the engine-vs-oracle-fp8 distance."""
    H, W, Lt, B, n = 64, 64, 32, 1, 16
    ts = fo.get_schedule(n, (H // 16) * (W // 16), shift=not schnell)
    tag = "schnell" if schnell else "dev"
    ref = {}
    for qname in QUANTS:
        cfg = tiny_config(schnell=schnell)
        model, sd = build(cfg, QUANTS[qname], dev)
        inp = inputs("plain", cfg.params, H, W, Lt, B, seed=7)
        if not ref:
            ref["o16"] = oracle_guided_loop(make_oracle(cfg, sd, None), inp, ts)
            with monkeypatch.context() as mp:
                mp.setattr(fo, "attention", fo.attention_exact)
                ref["o16x"] = oracle_guided_loop(make_oracle(cfg, sd, None), inp, ts)
            ref["floor16"] = rel_l2(ref["o16x"], ref["o16"])
        got = guided_denoise(model, to_dev(inp, dev), ts)
        assert got.shape == inp["img"].shape and torch.isfinite(got).all()
        e16 = rel_l2(got, ref["o16"])
        if qname == "bf16":
            gate = max(1e-2, 1.75 * ref["floor16"])
            print(f"[cfg {tag} bf16] engine vs oracle-bf16 {e16:.3e}; floor (oracle-bf16, exact attention) {ref['floor16']:.3e}; gate {gate:.3e}")
            assert e16 <= gate, f"{tag} bf16: rel-L2 {e16:.3e} > max(1e-2, 1.75 x {ref['floor16']:.3e})"
        else:
            o8 = oracle_guided_loop(make_oracle(cfg, sd, QUANTS[qname]), inp, ts)
            with monkeypatch.context() as mp:
                mp.setattr(fo, "attention", fo.attention_exact)
                o8x = oracle_guided_loop(make_oracle(cfg, sd, QUANTS[qname]), inp, ts)
            yard, floor8, e8 = rel_l2(o8, ref["o16"]), rel_l2(o8x, o8), rel_l2(got, o8)
            print(f"[cfg {tag} {qname}] engine vs oracle-bf16 {e16:.3e}; yardstick (oracle-fp8 vs oracle-bf16) {yard:.3e}; ratio {e16 / yard:.3f} "
                  f"(gate 1.25); engine vs oracle-fp8 {e8:.3e}; floor (oracle-fp8, exact attention) {floor8:.3e}")
            assert e16 <= 1.25 * yard, f"{tag} {qname}: vs bf16 flow {e16:.3e} > 1.25 x {yard:.3e}"


# ---- pipeline --------------------------------------------------------------------------------------------------------------------------
def test_pipeline_negative_prompt(dev, pipe):
    from PIL import Image

    pos, neg = prompts()
    kw = dict(width=64, height=96, num_steps=6, seed=7, silent=True)
    plain = pipe.generate(pos, output_type="latent", **kw)
    a = pipe.generate(pos, negative_prompt=neg, true_cfg_scale=SCALE, output_type="latent", **kw)
    b = pipe.generate(pos, negative_prompt=neg, true_cfg_scale=SCALE, output_type="latent", **kw)
    assert torch.equal(a, b), "same seed, different latents"
    assert a.shape == plain.shape and not torch.equal(a, plain)
    # a negative prompt with scale <= 1 is today's call, bit for bit (the negative prompt is not even encoded: a malformed one passes)
    assert torch.equal(pipe.generate(pos, negative_prompt=neg, true_cfg_scale=1.0, output_type="latent", **kw), plain)
    assert torch.equal(pipe.generate(pos, negative_prompt={"bogus": 1}, output_type="latent", **kw), plain)
    # == model.denoise on prepare's tensors: the generator's draw order is unchanged (same noise as the plain call)
    generator, _ = pipe.set_seed(7)
    noise, ts = pipe.preprocess_latent(height=96, width=64, num_steps=6, generator=generator, num_images=1)
    img, img_ids, vec, txt, txt_ids = map(lambda x: x.contiguous(), pipe.prepare(noise, pos))
    _, _, nvec, ntxt, _ = pipe.prepare(noise, neg)
    want = pipe.model.denoise(img, img_ids, txt, txt_ids, vec, ts, guidance=3.5, neg_txt=ntxt, neg_y=nvec, cfg_scale=SCALE)
    assert torch.equal(a, pipe.unpack(want.float(), 96, 64))
    # num_images = 2: one negative prompt for both, the two images' noise differs
    two = pipe.generate(pos, negative_prompt=neg, true_cfg_scale=SCALE, output_type="latent", num_images=2, **kw)
    assert two.shape[0] == 2 and not torch.equal(two[0], two[1])
    # through the VAE
    px = pipe.generate(pos, negative_prompt=neg, true_cfg_scale=SCALE, output_type="uint8", **kw)
    px = torch.as_tensor(px)
    assert px.dtype == torch.uint8 and tuple(px.shape) == (1, 96, 64, 3)
    assert torch.isfinite(a).all() and px.float().std() > 0
    buf = pipe.generate(pos, negative_prompt=neg, true_cfg_scale=SCALE, **kw)
    assert isinstance(buf, io.BytesIO) and Image.open(buf).size == (64, 96)


def test_pipeline_negative_prompt_composes_with_fill(dev):
    import numpy as np

    p = tiny_pipeline(dev, "fill")
    p.compile()
    pos, neg = prompts()
    rng = np.random.default_rng(0)
    photo = rng.integers(0, 256, size=(96, 64, 3), dtype=np.uint8)
    mask = np.zeros((96, 64), dtype=np.uint8)
    mask[24:72, 16:48] = 255
    kw = dict(init_image=photo, mask_image=mask, width=64, height=96, num_steps=6, seed=7, silent=True, output_type="latent")
    plain = p.generate(pos, **kw)
    a = p.generate(pos, negative_prompt=neg, true_cfg_scale=SCALE, **kw)
    assert a.shape == plain.shape and torch.isfinite(a).all() and not torch.equal(a, plain)
    generator, _ = p.set_seed(7)
    noise, ts = p.preprocess_latent(height=96, width=64, num_steps=6, generator=generator, num_images=1)
    img, img_ids, vec, txt, txt_ids = map(lambda x: x.contiguous(), p.prepare(noise, pos))
    _, _, nvec, ntxt, _ = p.prepare(noise, neg)
    cond = p.prepare_fill_conditioning(photo, mask, 96, 64, num_images=1, generator=generator)
    want = p.model.denoise(img, img_ids, txt, txt_ids, vec, ts, guidance=3.5, img_cond=cond, neg_txt=ntxt, neg_y=nvec, cfg_scale=SCALE)
    assert torch.equal(a, p.unpack(want.float(), 96, 64))


# ---- real width ------------------------------------------------------------------------------------------------------------------------
def test_guided_at_1024_real_width(dev):
    """hidden 3072, 1 + 1 blocks, 1024^2, Lt 512, one guided image (two samples in the engine): graph == eager, finite"""
    import util

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    cfg.params.depth, cfg.params.depth_single_blocks = 1, 1
    model, _ = build(cfg, QUANTS["fp8"], dev, seed=2)
    d = to_dev(inputs("plain", cfg.params, 1024, 1024, 512, 1, seed=8, real_tokens=64), dev)
    Li = d["img"].shape[1]
    assert Li + 512 == 4608
    ts = fo.get_schedule(16, Li)
    lat = guided_denoise(model, d, ts[:14], use_graph=False)  # calibrate at this shape
    assert model.calibration_state()[0] and torch.isfinite(lat).all()
    ts2 = ts[:5]
    a = guided_denoise(model, d, ts2, img=lat)
    b = guided_denoise(model, d, ts2, img=lat, use_graph=False)
    assert torch.isfinite(a).all() and torch.equal(a, b), f"graph vs eager: rel-L2 {rel_l2(a, b):.3e}"
    assert not torch.equal(a, plain_denoise(model, d, ts2, img=lat))
    print(f"[guided 1024^2 B=1] graph == eager; latents std {a.float().std().item():.3f}")
