"""FLUX.1 Kontext reference-image editing on the GPU: the engine's image stream carries the reference tokens behind the noisy ones
(fluxmi_engine_prepare_cond); only the noisy tokens are predicted and stepped.

The oracle needs no change: a Kontext step is oracle.forward(cat(img, cond), cat(ids, cond_ids), ...)[:, :Li] followed by the same bf16
Euler update as fo.denoise, calibrating steps included (img_in's running amax covers the reference rows, as in BFL's implementation).
Gates are those of tests/test_engine_gpu.py for the same flows.  The helpers below are copies of that file's."""
import io

import pytest
import torch

import flux_oracle as fo

pytestmark = pytest.mark.gpu


def tiny_config(schnell=False, **kw):
    import util

    cfg = util.load_config(util.ModelVersion.flux_schnell if schnell else util.ModelVersion.flux_dev, flow_dtype="bfloat16", **kw)
    p = cfg.params
    p.hidden_size, p.num_heads, p.depth, p.depth_single_blocks, p.context_in_dim, p.vec_in_dim = 256, 2, 2, 2, 128, 64
    return cfg


def build(cfg, quant, dev, seed=0):
    import util
    from float8_quantize import quantize_flow_transformer_and_dispatch_float8
    from fluxmi import synth

    sd = synth.make_state_dict(cfg.params, seed=seed)
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


def kontext_inputs(params, H, W, Lt, B, seed, grid, real_tokens=8):
    """synth.make_inputs + reference tokens on an (h, w) token grid: packed-latent-like N(0, 1) rows, ids with axis 0 = 1"""
    from flux_pipeline import kontext_reference_ids
    from fluxmi import synth

    inp = synth.make_inputs(params, H, W, Lt, batch=B, seed=seed, real_tokens=real_tokens)
    g = torch.Generator().manual_seed(500 + seed)
    h, w = grid
    inp["cond"] = torch.randn(B, h * w, params.in_channels, generator=g).to(torch.bfloat16)
    inp["cond_ids"] = kontext_reference_ids(B, 2 * h, 2 * w, "cpu", torch.bfloat16)
    return inp


def oracle_forward(oracle, inp, t, g):
    Li = inp["img"].shape[1]
    out = oracle.forward(torch.cat((inp["img"], inp["cond"]), 1), torch.cat((inp["img_ids"], inp["cond_ids"]), 1), inp["txt"], inp["txt_ids"],
                         t, inp["y"], g)
    return out[:, :Li]


def oracle_denoise(oracle, inp, timesteps, guidance=3.5):
    """fo.denoise with the reference tokens appended to every forward and only the noisy tokens stepped"""
    img = inp["img"]
    B = img.shape[0]
    g = torch.full((B,), guidance, dtype=oracle.dtype)
    for t_curr, t_prev in zip(timesteps[:-1], timesteps[1:]):
        t_vec = torch.full((B,), t_curr, dtype=oracle.dtype)
        pred = oracle_forward(oracle, {**inp, "img": img}, t_vec, g)
        img = img + (t_prev - t_curr) * pred
    return img


def kdenoise(model, d, ts, use_graph=True, img=None, cond=None):
    return model.denoise(d["img"] if img is None else img, d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts, guidance=3.5, use_graph=use_graph,
                         img_cond_seq=d["cond"] if cond is None else cond, img_cond_seq_ids=d["cond_ids"])


# ---- 1. forward vs the composed oracle through calibration ------------------------------------------------------------------------------
@pytest.mark.parametrize("qname", list(QUANTS))
@pytest.mark.parametrize("shape", [(64, 64, 32, 2, (3, 5)), (48, 80, 40, 1, (4, 6))])  # Li 16 / Lc 15 (odd); Li 15 / Lc 24
def test_forward_with_reference_matches_oracle_through_calibration(dev, qname, shape):
    H, W, Lt, B, grid = shape
    cfg = tiny_config()
    model, oracle, sd = build(cfg, QUANTS[qname], dev)
    oracle_bf16 = fo.FluxOracle({k: v.clone() for k, v in sd.items()}, fo.FluxParams(**cfg.params.model_dump()), quantize=None)
    inp = kontext_inputs(cfg.params, H, W, Lt, B, seed=3, grid=grid)
    d = to_dev(inp, dev)
    Li = inp["img"].shape[1]
    assert inp["cond"].shape[1] != Li
    worst = 0.0
    for step in range(15):
        t = torch.full((B,), 1.0 - 0.06 * step, dtype=torch.bfloat16)
        g = torch.full((B,), 3.5, dtype=torch.bfloat16)
        ref = oracle_forward(oracle, inp, t, g)
        got = model(d["img"], d["img_ids"], d["txt"], d["txt_ids"], t.to(dev), d["y"], g.to(dev), img_cond_seq=d["cond"],
                    img_cond_seq_ids=d["cond_ids"])
        assert got.shape == (B, Li, cfg.params.in_channels) and torch.isfinite(got).all()
        e = rel_l2(got, ref)
        worst = max(worst, e)
        if QUANTS[qname] is None:
            assert e <= 1e-2, f"{qname} call {step}: rel-L2 {e:.3e}"
        else:
            assert e <= 6e-2, f"{qname} call {step}: rel-L2 vs fp8 oracle {e:.3e}"
            if step in (0, 7, 14):
                rb = oracle_forward(oracle_bf16, inp, t, g)
                d_ref, d_got = rel_l2(ref, rb), rel_l2(got, rb)
                assert d_got <= 1.25 * d_ref, f"{qname} call {step}: vs bf16 flow {d_got:.3e} > 1.25 x {d_ref:.3e}"
    if QUANTS[qname] is not None:
        assert model.calibration_state()[0]
        names = [n for n, m in oracle.lin.items() if isinstance(m, fo.F8LinearState)]
        exact = 0
        for n in names:
            so, sg = oracle.lin[n].input_scale.item(), model.get_submodule(n).input_scale.item()
            assert abs(sg - so) <= 0.30 * so, f"{n}: input_scale {sg} vs oracle {so}"
            exact += int(sg == so)
        assert exact >= 0.3 * len(names), f"only {exact}/{len(names)} input scales bit-identical"
    print(f"[kontext {qname} {shape}] worst rel-L2 over 15 calls: {worst:.3e}")


# ---- 2. denoise vs the composed oracle loop ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schnell", [False, True])
def test_denoise_with_reference_matches_oracle(dev, schnell):
    for qname in ("bf16", "fp8"):
        cfg = tiny_config(schnell=schnell)
        model, oracle, _ = build(cfg, QUANTS[qname], dev)
        B, H, W, Lt = 1, 64, 64, 32
        inp = kontext_inputs(cfg.params, H, W, Lt, B, seed=7, grid=(3, 5))
        d = to_dev(inp, dev)
        n = 4 if schnell else 16
        ts = fo.get_schedule(n, (H // 16) * (W // 16), shift=not schnell)  # the noisy tokens only
        ref = oracle_denoise(oracle, inp, ts)
        got = kdenoise(model, d, ts)
        assert got.shape == inp["img"].shape
        e = rel_l2(got, ref)
        print(f"[kontext {qname} schnell={schnell}] latents after {n} steps: rel-L2 {e:.3e}")
        assert e <= (1e-2 if qname == "bf16" else 6e-2)


# ---- 3. bit-exactness -------------------------------------------------------------------------------------------------------------------
def test_reference_denoise_bit_exact(dev):
    import ctypes as C

    from fluxmi import _lib, ops, synth

    cfg = tiny_config()
    model, _, _ = build(cfg, QUANTS["fp8"], dev)
    B, H, W, Lt = 2, 64, 64, 32
    d = to_dev(kontext_inputs(cfg.params, H, W, Lt, B, seed=5, grid=(4, 4)), dev)  # Li 16 + Lc 16
    Li = d["img"].shape[1]
    cond0 = d["cond"].clone()
    ts = fo.get_schedule(16, Li)
    lat = kdenoise(model, d, ts[:14], use_graph=False)  # 13 calibrating steps
    assert model.calibration_state()[0] and lat.shape == d["img"].shape
    ts2 = ts[:9]
    a = kdenoise(model, d, ts2, img=lat)
    b = kdenoise(model, d, ts2, img=lat, use_graph=False)
    assert torch.equal(a, b), f"graph vs eager: rel-L2 {rel_l2(a, b):.3e}"
    c = lat.clone()
    g = torch.full((B,), 3.5, dtype=torch.bfloat16, device=dev)
    for t_curr, t_prev in zip(ts2[:-1], ts2[1:]):
        tv = torch.full((B,), t_curr, dtype=torch.bfloat16, device=dev)
        pred = model(c, d["img_ids"], d["txt"], d["txt_ids"], tv, d["y"], g, mode=1, img_cond_seq=d["cond"], img_cond_seq_ids=d["cond_ids"])
        c = c + (t_prev - t_curr) * pred
    assert torch.equal(a, c), f"graph loop vs python loop: rel-L2 {rel_l2(a, c):.3e}"
    assert torch.equal(d["cond"], cond0), "the caller's reference tokens changed"
    # the C entry on a caller-owned [B, Li + Lc, C] stream: the reference rows come back bit for bit, the noisy rows are the latents above
    full = torch.cat((lat, d["cond"]), 1).contiguous()
    txt, y = d["txt"].contiguous(), d["y"].contiguous()
    t_io = C.c_int(model._trial_counter())
    tsc = (C.c_double * len(ts2))(*ts2)
    with model._lock:
        _lib.call("fluxmi_engine_denoise", model._engine, ops._p(full), ops._p(txt), ops._p(y), 3.5, tsc, len(ts2) - 1, C.byref(t_io), 1,
                  ops._stream())
    assert torch.equal(full[:, Li:], cond0) and torch.equal(full[:, :Li], a)

    # one engine alternating a plain request and a Kontext request of the SAME image-stream length (32 rows: 16 + 16 vs a 64 x 128 image)
    plain = to_dev(synth.make_inputs(cfg.params, 64, 128, Lt, batch=B, seed=6, real_tokens=8), dev)
    assert plain["img"].shape[1] == Li + d["cond"].shape[1]
    pden = lambda: model.denoise(plain["img"], plain["img_ids"], plain["txt"], plain["txt_ids"], plain["y"], ts2, guidance=3.5)
    k1, p1 = kdenoise(model, d, ts2, img=lat), pden()
    k2, p2 = kdenoise(model, d, ts2, img=lat), pden()
    model._invalidate_engine()
    kf = kdenoise(model, d, ts2, img=lat)
    model._invalidate_engine()
    pf = pden()
    assert torch.equal(k1, a) and torch.equal(k2, kf) and torch.equal(k1, kf), "Kontext request after a plain one differs from a fresh engine"
    assert torch.equal(p1, p2) and torch.equal(p1, pf), "plain request after a Kontext one differs from a fresh engine"
    # every knob set of test_fused_equals_unfused_and_graph_equals_eager leaves the Kontext latents bit-identical
    for knobs in (dict(prefetch=0), dict(prefetch=2), dict(gemm_persist=0), dict(qlut=0), dict(fuse_kv=1), dict(fuse_kv=0), dict(w_pairs=0), dict(a_pairs=0)):
        with _lib.tuning(**knobs):
            a3 = kdenoise(model, d, ts2, img=lat)
        assert torch.equal(a, a3), f"Kontext latents change under tuning {knobs}: rel-L2 {rel_l2(a3, a):.3e}"


# ---- 4. real width, short sequence, against the oracle ---------------------------------------------------------------------------------
def test_full_width_with_reference_matches_oracle(dev):
    import util

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    p = cfg.params
    p.depth, p.depth_single_blocks = 1, 1
    model, oracle, _ = build(cfg, QUANTS["fp8"], dev, seed=1)
    B, Lt = 1, 64
    inp = kontext_inputs(p, 256, 256, Lt, B, seed=4, grid=(7, 11), real_tokens=16)  # Li 256 + Lc 77: L = 397
    d = to_dev(inp, dev)
    g = torch.full((B,), 3.5, dtype=torch.bfloat16)
    kw = dict(img_cond_seq=d["cond"], img_cond_seq_ids=d["cond_ids"])
    worst = 0.0
    for step in range(15):
        t = torch.full((B,), 1.0 - 0.05 * step, dtype=torch.bfloat16)
        ref = oracle_forward(oracle, inp, t, g)
        got = model(d["img"], d["img_ids"], d["txt"], d["txt_ids"], t.to(dev), d["y"], g.to(dev), **kw)
        assert torch.isfinite(got).all()
        e = rel_l2(got, ref)
        worst = max(worst, e)
        assert e <= 6e-2, f"full-width Kontext call {step}: rel-L2 vs fp8 oracle {e:.3e}"
    assert model.calibration_state()[0]
    t = torch.full((B,), 0.3, dtype=torch.bfloat16, device=dev)
    args = (d["img"], d["img_ids"], d["txt"], d["txt_ids"], t, d["y"], g.to(dev))
    a, b = model(*args, mode=1, **kw), model(*args, mode=2, **kw)
    assert rel_l2(a, b) <= 2e-3
    print(f"[full width, Kontext] worst rel-L2 over 15 calls: {worst:.3e}; fused vs unfused rel-L2 {rel_l2(a, b):.3e}")


# ---- 5. the headline Kontext shape, engine only -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref_grid", [(64, 64), (47, 87)])  # a 1024^2 reference (L = 8704) / a 1920 x 1080 one (Lc = 4089, L = 8697)
def test_headline_kontext_shape_at_real_width(dev, ref_grid):
    import util

    from fluxmi import ops

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    p = cfg.params
    p.depth, p.depth_single_blocks = 1, 1
    model, _, _ = build(cfg, QUANTS["fp8"], dev, seed=2)
    B, Lt = 2, 512
    inp = kontext_inputs(p, 1024, 1024, Lt, B, seed=8, grid=ref_grid, real_tokens=64)
    d = to_dev(inp, dev)
    Li, Lc = d["img"].shape[1], d["cond"].shape[1]
    L = Lt + Li + Lc
    assert L == {(64, 64): 8704, (47, 87): 8697}[ref_grid]
    # the attention plan at this length: 34 row blocks x 24 heads = 816 tasks per sample = 102 per XCD, a thin last round of 6 of 32 CUs --
    # but the balanced grid would need 70 pieces per XCD (> ATTN_MAX_PIECES = 64), so there is no plan and attention runs one workgroup
    # per task (the partial-state scratch is not allocated)
    assert ops.attention_plan(1, L, 24) is None and ops.attention_plan(B, L, 24) is None
    ts = fo.get_schedule(16, Li)
    lat = kdenoise(model, d, ts[:14], use_graph=False)  # calibrate at this shape
    assert model.calibration_state()[0] and torch.isfinite(lat).all()
    ts2 = ts[:5]
    a = kdenoise(model, d, ts2, img=lat)
    b = kdenoise(model, d, ts2, img=lat, use_graph=False)
    assert torch.isfinite(a).all() and torch.equal(a, b), f"graph vs eager at L = {L}: rel-L2 {rel_l2(a, b):.3e}"
    # batch invariance: sample 0 alone == sample 0 beside a DIFFERENT second reference
    one = {k: v[:1] for k, v in d.items()}
    a1 = kdenoise(model, one, ts2, img=lat[:1])
    other = d["cond"].clone()
    other[1] = torch.randn(other.shape[1:], generator=torch.Generator().manual_seed(99)).to(other)
    a2 = kdenoise(model, d, ts2, img=lat, cond=other)
    assert torch.equal(a1[0], a[0]) and torch.equal(a2[0], a[0]), "sample 0 depends on its batch"
    assert not torch.equal(a2[1], a[1])
    print(f"[headline Kontext L={L}] graph == eager, batch-invariant; latents std {a.float().std().item():.3f}")


@pytest.mark.parametrize("attn_split", [0, 2])
def test_attention_at_the_kontext_length_vs_fp64(dev, attn_split):
    """The attention op alone at L = 8704, 24 heads, against an fp64 softmax on sampled query rows, with the balanced grid off and forced
    on (attn_split = 2: wherever a plan exists -- there is none at this length, so both launch one workgroup per task)."""
    import math

    from fluxmi import _lib, ops

    B, H, L = 1, 24, 8704
    torch.manual_seed(87)
    q = torch.randn(B, H, L, 128).bfloat16()
    k = torch.randn(B, H, L, 128).bfloat16()
    v = torch.randn(B, H, L, 128).bfloat16()
    Lp = (L + 63) // 64 * 64
    pos = torch.arange(Lp)
    j = pos % 16
    key = (pos // 16) * 16 + ((j & 3) | (((j >> 2) & 1) << 3) | (((j >> 3) & 1) << 2))
    vpad = torch.zeros(B, H, Lp, 128, dtype=torch.bfloat16)
    vpad[:, :, :L] = v
    VT = vpad[:, :, key].transpose(-1, -2).contiguous()  # the kernels' V^T layout (copy of tests/test_ops_gpu.py::_vt_layout)
    with _lib.tuning(attn_split=attn_split):
        out = ops.attention(q.to(dev), k.half().to(dev), VT.to(dev)).cpu()
    assert torch.isfinite(out).all()
    g = torch.Generator().manual_seed(3)
    vmax = v.abs().max().item()
    worst = 0.0
    for h in (0, 11, 23):
        rows = torch.cat((torch.tensor([0, 255, 256, L - 1]), torch.randint(0, L, (28,), generator=g)))
        s = (q[0, h, rows].double() @ k[0, h].double().T) / math.sqrt(128)
        ref = torch.softmax(s, -1) @ v[0, h].double()
        got = out[0, rows, h * 128:(h + 1) * 128].double()
        err = (got - ref).abs().max().item()
        worst = max(worst, err)
        assert err <= 2e-2 * vmax, f"head {h}: max |err| {err:.3e}"
    print(f"attention L={L} attn_split={attn_split}: max |err| vs fp64 on sampled rows {worst:.3e}")


# ---- 6. pipeline end to end through the tiny VAE --------------------------------------------------------------------------------------
def test_pipeline_kontext_through_vae(dev, tmp_path):
    import base64

    import numpy as np
    from PIL import Image

    from flux_pipeline import FluxPipeline
    from fluxmi import synth
    from modules.autoencoder import AutoEncoder, AutoEncoderParams

    cfg = tiny_config()
    cfg.text_enc_max_length = 32
    cfg.ae_device = str(dev)
    cfg.ae_params = AutoEncoderParams(resolution=32, in_channels=3, ch=32, out_ch=3, ch_mult=[1, 2, 2, 2], num_res_blocks=1, z_channels=16,
                                      scale_factor=0.3611, shift_factor=0.1159)
    torch.manual_seed(0)
    ae_sd = {k: v.clone() for k, v in AutoEncoder(cfg.ae_params).state_dict().items()}
    pipe = FluxPipeline.load_pipeline_from_config(cfg, state_dict=synth.make_state_dict(cfg.params, seed=0), ae_state_dict=ae_sd)
    pipe.compile()
    g = torch.Generator().manual_seed(1)
    prompt = {"txt": 0.1 * torch.randn(1, 32, 128, generator=g), "vec": torch.randn(1, 64, generator=g)}
    rng = np.random.default_rng(0)
    ref = rng.integers(0, 256, size=(90, 160, 3), dtype=np.uint8)  # 16:9 -> 1392 x 752, Lc = 4089
    path = tmp_path / "ref.png"
    Image.fromarray(ref).save(path)
    b64 = base64.b64encode(path.read_bytes()).decode()
    kw = dict(width=64, height=96, num_steps=6, seed=7, silent=True)
    outs = []
    for src in (ref, Image.fromarray(ref), torch.from_numpy(ref), str(path), b64):
        buf = pipe.generate(prompt, reference_image=src, **kw)
        assert isinstance(buf, io.BytesIO)
        im = Image.open(buf)
        assert im.size == (64, 96) and im.mode == "RGB"
        outs.append(buf.getvalue())
    assert all(o == outs[0] for o in outs), "the input formats give different results"
    again = pipe.generate(prompt, reference_image=ref, **kw).getvalue()
    assert again == outs[0], "same seed, different bytes"
    plain = pipe.generate(prompt, **kw).getvalue()
    assert plain != outs[0]
    two = pipe.generate(prompt, reference_image=ref, num_images=2, **kw)
    assert Image.open(two).size == (64, 2 * 96)
    # output_type="latent" == model.denoise fed the same noise and the preprocessed reference (drawn in generate's order: noise, then the
    # VAE sample of the reference, from the request's generator)
    lat = pipe.generate(prompt, reference_image=ref, output_type="latent", **kw)
    generator, _ = pipe.set_seed(7)
    noise, ts = pipe.preprocess_latent(height=96, width=64, num_steps=6, generator=generator, num_images=1)
    img, img_ids, vec, txt, txt_ids = map(lambda x: x.contiguous(), pipe.prepare(noise, prompt))
    cond, cond_ids = pipe.prepare_kontext_reference(ref, num_images=1, generator=generator)
    assert cond.shape == (1, 4089, 64) and cond_ids.shape == (1, 4089, 3) and (cond_ids[..., 0] == 1).all()
    want = pipe.model.denoise(img, img_ids, txt, txt_ids, vec, ts, guidance=3.5, img_cond_seq=cond, img_cond_seq_ids=cond_ids)
    assert torch.equal(lat, pipe.unpack(want.float(), 96, 64))
    # init_image / strength compose with a reference
    buf = pipe.generate(prompt, reference_image=ref, init_image=ref, strength=0.5, **kw)
    assert Image.open(buf).size == (64, 96)


def test_vae_attention_at_a_pixel_count_off_the_8_grid(dev):
    """The 1392 x 752 Kontext reference has a 174 x 94 latent: 16356 pixels, no multiple of 8, which the VAE's mid-block attention now runs
    padded (masked keys).  The native encoder at such a size (48 x 80 -> a 6 x 10 latent, 60 pixels) against the oracle encoder."""
    import vae_oracle as vo
    from modules.autoencoder import AutoEncoder, AutoEncoderParams

    params = dict(resolution=32, in_channels=3, ch=32, out_ch=3, ch_mult=[1, 2, 2, 2], num_res_blocks=1, z_channels=16, scale_factor=0.3611,
                  shift_factor=0.1159)
    torch.manual_seed(0)
    ae = AutoEncoder(AutoEncoderParams(**params))
    sd = {k: v.clone() for k, v in ae.state_dict().items()}
    ae.to(dev)
    x = torch.rand(1, 3, 48, 80, generator=torch.Generator().manual_seed(2)) * 2 - 1
    mom = ae.encode_moments(x.to(dev)).float().cpu()
    ref = vo.encode_moments(sd, params, x, autocast=True).float()
    assert mom.shape == ref.shape == (1, 32, 6, 10) and torch.isfinite(mom).all()
    e = rel_l2(mom, ref)
    print(f"VAE encode at a 6 x 10 latent: native vs oracle-autocast rel-L2 {e:.3e}")
    assert e <= 2e-2
