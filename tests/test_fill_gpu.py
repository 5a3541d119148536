"""FLUX.1 Fill / Depth / Canny on the GPU: the engine's image stream is C_in channels wide, the trailing C_in - C_out are step-invariant
conditioning; only the leading C_out channels are predicted and stepped.

The oracle needs no change: it builds every linear from the weight shapes, so a conditioned step is oracle.forward(cat(img, img_cond, -1),
...) followed by the same bf16 Euler update as fo.denoise on the C_out noisy channels, calibrating steps included (img_in's running amax
covers the conditioning channels, as in BFL's implementation).  Gates are those of tests/test_engine_gpu.py for the same flows."""
import io

import pytest
import torch

import flux_oracle as fo

pytestmark = pytest.mark.gpu

KINDS = {"fill": 384, "control": 128}


def tiny_config(kind="fill", schnell=False):
    import util

    cfg = util.load_config(util.ModelVersion.flux_schnell if schnell else util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    p = cfg.params
    p.hidden_size, p.num_heads, p.depth, p.depth_single_blocks, p.context_in_dim, p.vec_in_dim = 256, 2, 2, 2, 128, 64
    p.in_channels, p.out_channels = KINDS[kind], 64
    return cfg


def conditioned_state_dict(params, seed):
    """The text-to-image test model of tests/test_engine_gpu.py (same seed, every weight the same) plus img_in columns for the conditioning
    channels, drawn as synth draws a linear of the wider K -- as BFL's Fill / Depth / Canny are Flux-dev with a wider img_in.  With zero
    conditioning this IS the plain test model, whose fp8 noise the gates were set on.  (A test model whose noisy-channel columns are drawn at
    the wider K's bound, as synth.make_state_dict at in_channels 384 does, embeds the noisy tokens at sqrt(64 / 384) of their plain
    amplitude; that alone, with the conditioning zeroed, raises the tiny model's fp8-vs-oracle distance to 7-10e-2.)"""
    import math

    from fluxmi import synth

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

    sd = conditioned_state_dict(cfg.params, seed)
    model = util.load_flow_model(cfg, {k: v.clone() for k, v in sd.items()})
    model.to(dev)
    if quant is not None:
        quantize_flow_transformer_and_dispatch_float8(model, dev, flow_dtype=torch.bfloat16, swap_linears_with_cublaslinear=False,
                                                      quantize_modulation=quant["modulation"], quantize_flow_embedder_layers=quant["embedders"])
    oracle = fo.FluxOracle({k: v.clone() for k, v in sd.items()}, fo.FluxParams(**cfg.params.model_dump()), quantize=quant)
    return model, oracle, sd


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


def fill_inputs(params, H, W, Lt, B, seed, real_tokens=8):
    """synth.make_inputs + conditioning channels: N(0, 1) latent-like channels, then (Fill) the packed mask of one rectangle per sample
    (FluxPipeline.pack_fill_mask of an H x W pixel mask, as an inpainting request has)"""
    from flux_pipeline import FluxPipeline
    from fluxmi import synth

    inp = synth.make_inputs(params, H, W, Lt, batch=B, seed=seed, real_tokens=real_tokens)
    g = torch.Generator().manual_seed(500 + seed)
    Li, extra = inp["img"].shape[1], params.in_channels - params.out_channels
    cond = torch.randn(B, Li, 64, generator=g).to(torch.bfloat16)
    if extra > 64:
        m = torch.zeros(B, 1, H, W)
        for b in range(B):
            y0, x0 = int(torch.randint(0, H // 2, (1,), generator=g)), int(torch.randint(0, W // 2, (1,), generator=g))
            m[b, :, y0:y0 + H // 2 + 3, x0:x0 + W // 3 + 5] = 1.0
        cond = torch.cat((cond, FluxPipeline.pack_fill_mask(m)), -1)
    assert cond.shape == (B, Li, extra)
    inp["cond"] = cond
    return inp


def oracle_forward(oracle, inp, t, g, img=None):
    img = inp["img"] if img is None else img
    return oracle.forward(torch.cat((img, inp["cond"]), -1), inp["img_ids"], inp["txt"], inp["txt_ids"], t, inp["y"], g)


def oracle_denoise(oracle, inp, timesteps, guidance=3.5):
    """fo.denoise with the conditioning channels appended to every forward and only the noisy channels stepped"""
    img = inp["img"]
    B = img.shape[0]
    g = torch.full((B,), guidance, dtype=oracle.dtype)
    for t_curr, t_prev in zip(timesteps[:-1], timesteps[1:]):
        t_vec = torch.full((B,), t_curr, dtype=oracle.dtype)
        img = img + (t_prev - t_curr) * oracle_forward(oracle, inp, t_vec, g, img=img)
    return img


def fdenoise(model, d, ts, use_graph=True, img=None, cond=None):
    return model.denoise(d["img"] if img is None else img, d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts, guidance=3.5, use_graph=use_graph,
                         img_cond=d["cond"] if cond is None else cond)


# ---- 1. forward vs the oracle through calibration ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("qname", list(QUANTS))
@pytest.mark.parametrize("shape", [(64, 64, 32, 2), (48, 80, 40, 1)])  # Li 16, B 2; Li 15 (odd), B 1
def test_forward_with_channels_matches_oracle_through_calibration(dev, kind, qname, shape):
    """The gates of test_engine_gpu.py / test_kontext_gpu.py for the same flows: bf16 rel-L2 <= 1e-2 per call; fp8 rel-L2 <= 6e-2 against
    the fp8 oracle per call, SURVEY.md §8c gate (iv) at calls 0 / 7 / 14, every calibrated input scale within 30 % of the oracle's and at
    least 30 % of them bit-identical (img_in's among them with fp8 embedders: its amax covers the conditioning channels)."""
    H, W, Lt, B = shape
    cfg = tiny_config(kind)
    model, oracle, sd = build(cfg, QUANTS[qname], dev)
    oracle_bf16 = None if QUANTS[qname] is None else fo.FluxOracle({k: v.clone() for k, v in sd.items()},
                                                                   fo.FluxParams(**cfg.params.model_dump()), quantize=None)
    inp = fill_inputs(cfg.params, H, W, Lt, B, seed=3)
    d = to_dev(inp, dev)
    Li = inp["img"].shape[1]
    worst = 0.0
    for step in range(15):
        t = torch.full((B,), 1.0 - 0.06 * step, dtype=torch.bfloat16)
        g = torch.full((B,), 3.5, dtype=torch.bfloat16)
        ref = oracle_forward(oracle, inp, t, g)
        got = model(d["img"], d["img_ids"], d["txt"], d["txt_ids"], t.to(dev), d["y"], g.to(dev), img_cond=d["cond"])
        assert got.shape == (B, Li, 64) and ref.shape == got.shape and torch.isfinite(got).all()
        e = rel_l2(got, ref)
        worst = max(worst, e)
        if oracle_bf16 is None:
            assert e <= 1e-2, f"{kind} {qname} call {step}: rel-L2 {e:.3e}"
        else:
            assert e <= 6e-2, f"{kind} {qname} call {step}: rel-L2 vs fp8 oracle {e:.3e}"
            if step in (0, 7, 14):
                rb = oracle_forward(oracle_bf16, inp, t, g)
                d_ref, d_got = rel_l2(ref, rb), rel_l2(got, rb)
                assert d_got <= 1.25 * d_ref, f"{kind} {qname} call {step}: vs bf16 flow {d_got:.3e} > 1.25 x {d_ref:.3e}"
    if QUANTS[qname] is not None:
        assert model.calibration_state()[0]
        names = [n for n, m in oracle.lin.items() if isinstance(m, fo.F8LinearState)]
        assert ("img_in" in names) == QUANTS[qname]["embedders"]
        exact = 0
        for n in names:
            so, sg = oracle.lin[n].input_scale.item(), model.get_submodule(n).input_scale.item()
            assert abs(sg - so) <= 0.30 * so, f"{n}: input_scale {sg} vs oracle {so}"
            exact += int(sg == so)
        assert exact >= 0.3 * len(names), f"only {exact}/{len(names)} input scales bit-identical"
    print(f"[{kind} {qname} {shape}] worst rel-L2 over 15 calls: {worst:.3e}")


# ---- 2. denoise vs the composed oracle loop ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("schnell", [False, True])
def test_denoise_with_channels_matches_oracle(dev, schnell):
    for qname in ("bf16", "fp8", "fp8_emb"):
        cfg = tiny_config("fill", schnell=schnell)
        model, oracle, _ = build(cfg, QUANTS[qname], dev)
        B, H, W, Lt = 1, 64, 64, 32
        inp = fill_inputs(cfg.params, H, W, Lt, B, seed=7)
        d = to_dev(inp, dev)
        n = 4 if schnell else 16
        ts = fo.get_schedule(n, (H // 16) * (W // 16), shift=not schnell)
        ref = oracle_denoise(oracle, inp, ts)
        got = fdenoise(model, d, ts)
        assert got.shape == inp["img"].shape
        e = rel_l2(got, ref)
        print(f"[fill {qname} schnell={schnell}] latents after {n} steps: rel-L2 {e:.3e}")
        assert e <= (1e-2 if qname == "bf16" else 6e-2)


# ---- 3. bit-exactness -----------------------------------------------------------------------------------------------------------------
def test_fill_denoise_bit_exact(dev):
    import ctypes as C

    from fluxmi import _lib, ops

    cfg = tiny_config("fill")
    model, _, _ = build(cfg, QUANTS["fp8"], dev)
    B, H, W, Lt = 2, 64, 64, 32
    d = to_dev(fill_inputs(cfg.params, H, W, Lt, B, seed=5), dev)
    Li = d["img"].shape[1]
    cond0 = d["cond"].clone()
    ts = fo.get_schedule(16, Li)
    lat = fdenoise(model, d, ts[:14], use_graph=False)  # 13 calibrating steps
    assert model.calibration_state()[0] and lat.shape == d["img"].shape
    ts2 = ts[:9]
    a = fdenoise(model, d, ts2, img=lat)
    b = fdenoise(model, d, ts2, img=lat, use_graph=False)
    assert torch.equal(a, b), f"graph vs eager: rel-L2 {rel_l2(a, b):.3e}"
    c = lat.clone()
    g = torch.full((B,), 3.5, dtype=torch.bfloat16, device=dev)
    for t_curr, t_prev in zip(ts2[:-1], ts2[1:]):
        tv = torch.full((B,), t_curr, dtype=torch.bfloat16, device=dev)
        c = c + (t_prev - t_curr) * model(c, d["img_ids"], d["txt"], d["txt_ids"], tv, d["y"], g, mode=1, img_cond=d["cond"])
    assert torch.equal(a, c), f"graph loop vs python loop: rel-L2 {rel_l2(a, c):.3e}"
    assert torch.equal(d["cond"], cond0), "the caller's conditioning changed"
    # the C entry on a caller-owned [B, Li, C_in] stream: the conditioning channels come back bit for bit
    full = torch.cat((lat, d["cond"]), -1).contiguous()
    txt, y = d["txt"].contiguous(), d["y"].contiguous()
    t_io = C.c_int(model._trial_counter())
    tsc = (C.c_double * len(ts2))(*ts2)
    with model._lock:
        _lib.call("fluxmi_engine_denoise", model._engine, ops._p(full), ops._p(txt), ops._p(y), 3.5, tsc, len(ts2) - 1, C.byref(t_io), 1,
                  ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(full[..., 64:], cond0) and torch.equal(full[..., :64], a)
    # a Kontext row split on a channel-conditioned engine is refused
    ids = torch.cat((d["img_ids"], d["img_ids"][:, :3]), 1).contiguous()
    with model._lock, pytest.raises(RuntimeError, match="in_channels == out_channels"):
        _lib.call("fluxmi_engine_prepare_cond", model._engine, B, Li, 3, Lt, ops._p(ids), ops._p(d["txt_ids"].contiguous()), ops._stream())
    # one engine alternating two image sizes (re-allocation + re-capture) == fresh engines
    d2 = to_dev(fill_inputs(cfg.params, 48, 80, Lt, B, seed=6), dev)
    a1, o1 = fdenoise(model, d, ts2, img=lat), fdenoise(model, d2, ts2)
    a2, o2 = fdenoise(model, d, ts2, img=lat), fdenoise(model, d2, ts2)
    model._invalidate_engine()
    of = fdenoise(model, d2, ts2)
    model._invalidate_engine()
    af = fdenoise(model, d, ts2, img=lat)
    assert torch.equal(a1, a) and torch.equal(a2, a) and torch.equal(af, a), "a size change and back differs from a fresh engine"
    assert torch.equal(o1, o2) and torch.equal(o1, of)
    # the knob sets of the Kontext test leave Fill latents bit-identical
    for knobs in (dict(prefetch=0), dict(prefetch=2), dict(gemm_persist=0), dict(qlut=0), dict(fuse_kv=1), dict(fuse_kv=0), dict(w_pairs=0), dict(a_pairs=0)):
        with _lib.tuning(**knobs):
            a3 = fdenoise(model, d, ts2, img=lat)
        assert torch.equal(a, a3), f"Fill latents change under tuning {knobs}: rel-L2 {rel_l2(a3, a):.3e}"


# ---- 4. real width -----------------------------------------------------------------------------------------------------------------
def full_width(kind, dev, seed):
    import util

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    p = cfg.params
    p.depth, p.depth_single_blocks = 1, 1
    p.in_channels, p.out_channels = KINDS[kind], 64
    return cfg, build(cfg, QUANTS["fp8"], dev, seed=seed)


def test_full_width_fill_matches_oracle(dev):
    cfg, (model, oracle, _) = full_width("fill", dev, seed=1)
    B, Lt = 1, 64
    inp = fill_inputs(cfg.params, 256, 256, Lt, B, seed=4, real_tokens=16)
    d = to_dev(inp, dev)
    g = torch.full((B,), 3.5, dtype=torch.bfloat16)
    worst = 0.0
    for step in range(15):
        t = torch.full((B,), 1.0 - 0.05 * step, dtype=torch.bfloat16)
        ref = oracle_forward(oracle, inp, t, g)
        got = model(d["img"], d["img_ids"], d["txt"], d["txt_ids"], t.to(dev), d["y"], g.to(dev), img_cond=d["cond"])
        assert torch.isfinite(got).all()
        e = rel_l2(got, ref)
        worst = max(worst, e)
        assert e <= 6e-2, f"full-width Fill call {step}: rel-L2 vs fp8 oracle {e:.3e}"
    assert model.calibration_state()[0]
    t = torch.full((B,), 0.3, dtype=torch.bfloat16, device=dev)
    args = (d["img"], d["img_ids"], d["txt"], d["txt_ids"], t, d["y"], g.to(dev))
    a, b = model(*args, mode=1, img_cond=d["cond"]), model(*args, mode=2, img_cond=d["cond"])
    assert rel_l2(a, b) <= 2e-3
    print(f"[full width, Fill] worst rel-L2 over 15 calls: {worst:.3e}; fused vs unfused rel-L2 {rel_l2(a, b):.3e}")


def test_fill_at_1024_real_width(dev):
    cfg, (model, _, _) = full_width("fill", dev, seed=2)
    B, Lt = 2, 512
    d = to_dev(fill_inputs(cfg.params, 1024, 1024, Lt, B, seed=8, real_tokens=64), dev)
    Li = d["img"].shape[1]
    assert Li + Lt == 4608
    ts = fo.get_schedule(16, Li)
    lat = fdenoise(model, d, ts[:14], use_graph=False)  # calibrate at this shape
    assert model.calibration_state()[0] and torch.isfinite(lat).all()
    ts2 = ts[:5]
    a = fdenoise(model, d, ts2, img=lat)
    b = fdenoise(model, d, ts2, img=lat, use_graph=False)
    assert torch.isfinite(a).all() and torch.equal(a, b), f"graph vs eager: rel-L2 {rel_l2(a, b):.3e}"
    # batch invariance: sample 0 alone == sample 0 beside a DIFFERENT second mask
    one = {k: v[:1] for k, v in d.items()}
    a1 = fdenoise(model, one, ts2, img=lat[:1])
    other = d["cond"].clone()
    other[1, :, 64:] = 1 - other[1, :, 64:]
    a2 = fdenoise(model, d, ts2, img=lat, cond=other)
    assert torch.equal(a1[0], a[0]) and torch.equal(a2[0], a[0]), "sample 0 depends on its batch"
    assert not torch.equal(a2[1], a[1])
    print(f"[Fill 1024^2 B=2] graph == eager, batch-invariant; latents std {a.float().std().item():.3f}")


# ---- 5. pipeline end to end through the tiny VAE ------------------------------------------------------------------------------------
def tiny_pipeline(dev, kind):
    from flux_pipeline import FluxPipeline
    from fluxmi import synth
    from modules.autoencoder import AutoEncoder, AutoEncoderParams

    cfg = tiny_config(kind) if kind else tiny_config("fill")
    if kind is None:
        cfg.params.in_channels, cfg.params.out_channels = 64, None
    cfg.text_enc_max_length = 32
    cfg.ae_device = str(dev)
    cfg.ae_params = AutoEncoderParams(resolution=32, in_channels=3, ch=32, out_ch=3, ch_mult=[1, 2, 2, 2], num_res_blocks=1, z_channels=16,
                                      scale_factor=0.3611, shift_factor=0.1159)
    torch.manual_seed(0)
    ae_sd = {k: v.clone() for k, v in AutoEncoder(cfg.ae_params).state_dict().items()}
    return FluxPipeline.load_pipeline_from_config(cfg, state_dict=synth.make_state_dict(cfg.params, seed=0), ae_state_dict=ae_sd)


def test_pipeline_fill_through_vae(dev, tmp_path):
    import base64

    import numpy as np
    from PIL import Image

    pipe = tiny_pipeline(dev, "fill")
    assert pipe.conditioning_kind() == "fill"
    pipe.compile()
    assert pipe.model.calibration_state()[0], "compile() must freeze the input scales of a Fill model"
    g = torch.Generator().manual_seed(1)
    prompt = {"txt": 0.1 * torch.randn(1, 32, 128, generator=g), "vec": torch.randn(1, 64, generator=g)}
    rng = np.random.default_rng(0)
    photo = rng.integers(0, 256, size=(96, 64, 3), dtype=np.uint8)
    mask = np.zeros((96, 64), dtype=np.uint8)
    mask[24:72, 16:48] = 255
    path = tmp_path / "mask.png"
    Image.fromarray(mask).save(path)
    b64 = base64.b64encode(path.read_bytes()).decode()
    kw = dict(init_image=photo, width=64, height=96, num_steps=6, seed=7, silent=True)
    outs = []
    for src in (mask, Image.fromarray(mask), torch.from_numpy(mask), str(path), b64):
        buf = pipe.generate(prompt, mask_image=src, **kw)
        assert isinstance(buf, io.BytesIO)
        im = Image.open(buf)
        assert im.size == (64, 96) and im.mode == "RGB"
        outs.append(buf.getvalue())
    assert all(o == outs[0] for o in outs), "the mask's input forms give different results"
    # ... and the image to inpaint in every form (PNG: lossless)
    ppath = tmp_path / "photo.png"
    Image.fromarray(photo).save(ppath)
    pb64 = "data:image/png;base64," + base64.b64encode(ppath.read_bytes()).decode()
    kw_no_init = {k: v for k, v in kw.items() if k != "init_image"}
    for src in (Image.fromarray(photo), torch.from_numpy(photo), str(ppath), pb64):
        assert pipe.generate(prompt, init_image=src, mask_image=mask, **kw_no_init).getvalue() == outs[0], "the image's input forms differ"
    assert pipe.generate(prompt, mask_image=mask, **kw).getvalue() == outs[0], "same seed, different bytes"
    black, white = np.zeros_like(mask), np.full_like(mask, 255)
    assert pipe.generate(prompt, mask_image=black, **kw).getvalue() != pipe.generate(prompt, mask_image=white, **kw).getvalue()
    # output_type="latent" == model.denoise fed generate's RNG order: the noise, then the VAE sample of the masked image
    lat = pipe.generate(prompt, mask_image=mask, output_type="latent", **kw)
    generator, _ = pipe.set_seed(7)
    noise, ts = pipe.preprocess_latent(height=96, width=64, num_steps=6, generator=generator, num_images=1)
    img, img_ids, vec, txt, txt_ids = map(lambda x: x.contiguous(), pipe.prepare(noise, prompt))
    cond = pipe.prepare_fill_conditioning(photo, mask, 96, 64, num_images=1, generator=generator)
    assert cond.shape == (1, 24, 320) and cond.dtype == torch.bfloat16
    want = pipe.model.denoise(img, img_ids, txt, txt_ids, vec, ts, guidance=3.5, img_cond=cond)
    assert torch.equal(lat, pipe.unpack(want.float(), 96, 64))
    # strength < 1 composes as img2img: init_image's latents blended into the start at t_idx = int(0.5 * 6) = 3, then the same Fill steps.
    # The img2img encode draws its Gaussian sample from the global RNG (as the reference's does): seeded here for both sides.
    torch.manual_seed(5)
    half = pipe.generate(prompt, mask_image=mask, strength=0.5, output_type="latent", **kw)
    torch.manual_seed(5)
    generator, _ = pipe.set_seed(7)
    noise, ts_h = pipe.preprocess_latent(init_image=pipe.load_init_image_if_needed(photo), height=96, width=64, num_steps=6, strength=0.5,
                                         generator=generator, num_images=1)
    assert len(ts_h) == 4 and ts_h == ts[3:]
    img, img_ids, vec, txt, txt_ids = map(lambda x: x.contiguous(), pipe.prepare(noise, prompt))
    cond = pipe.prepare_fill_conditioning(photo, mask, 96, 64, num_images=1, generator=generator)
    want = pipe.model.denoise(img, img_ids, txt, txt_ids, vec, ts_h, guidance=3.5, img_cond=cond)
    assert torch.equal(half, pipe.unpack(want.float(), 96, 64)) and not torch.equal(half, lat)
    assert Image.open(pipe.generate(prompt, mask_image=mask, strength=0.5, **kw)).size == (64, 96)
    assert Image.open(pipe.generate(prompt, mask_image=mask, num_images=2, **kw)).size == (64, 2 * 96)
    with pytest.raises(ValueError, match="mask_image"):
        pipe.generate(prompt, **kw)
    with pytest.raises(ValueError, match="control_image"):
        pipe.generate(prompt, mask_image=mask, control_image=photo, **kw)


def test_pipeline_control_and_plain_refusals(dev, tmp_path):
    import base64

    import numpy as np
    from PIL import Image

    g = torch.Generator().manual_seed(1)
    prompt = {"txt": 0.1 * torch.randn(1, 32, 128, generator=g), "vec": torch.randn(1, 64, generator=g)}
    depth = np.tile(np.linspace(0, 255, 64, dtype=np.uint8)[None, :, None], (96, 1, 3))
    kw = dict(width=64, height=96, num_steps=6, seed=3, silent=True)
    pipe = tiny_pipeline(dev, "control")
    assert pipe.conditioning_kind() == "control"
    pipe.compile()
    assert pipe.model.calibration_state()[0]
    a = pipe.generate(prompt, control_image=depth, **kw).getvalue()
    assert Image.open(io.BytesIO(a)).size == (64, 96)
    path = tmp_path / "depth.png"
    Image.fromarray(depth).save(path)
    b64 = base64.b64encode(path.read_bytes()).decode()
    for src in (Image.fromarray(depth), torch.from_numpy(depth), str(path), b64):
        assert pipe.generate(prompt, control_image=src, **kw).getvalue() == a, "the control image's input forms differ"
    assert pipe.generate(prompt, control_image=255 - depth, **kw).getvalue() != a
    with pytest.raises(ValueError, match="control_image"):
        pipe.generate(prompt, **kw)
    plain = tiny_pipeline(dev, None)
    assert plain.conditioning_kind() is None
    with pytest.raises(ValueError, match="no conditioning channels"):
        plain.generate(prompt, init_image=depth, mask_image=depth[..., 0], **kw)
    with pytest.raises(ValueError, match="no conditioning channels"):
        plain.generate(prompt, control_image=depth, **kw)
