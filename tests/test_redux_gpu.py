"""FLUX.1 Redux on the GPU: the vision-attention and patch-embedding kernels, the native SigLIP and the projector against transformers /
fp32, the engine at the odd text lengths Redux produces (Lt = 512 + 729 = 1241 for dev), and the pipeline end to end.

The engine needs no Redux-specific code: Redux only lengthens the text stream.  Its odd-Lt tests are the gates of tests/test_engine_gpu.py
for the same flows, used as tests/test_kontext_gpu.py uses them; the helpers below are copies of that file's."""
import math

import numpy as np
import pytest
import torch

import flux_oracle as fo

pytestmark = pytest.mark.gpu

TINY = dict(hidden_size=144, intermediate_size=344, num_hidden_layers=3, num_attention_heads=2, image_size=384, patch_size=14,
            num_channels=3, hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-6)


def rel_l2(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def to_dev(inp, dev):
    return {k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in inp.items()}


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


QUANTS = {
    "bf16": None,
    "fp8": dict(modulation=True, embedders=False),
    "fp8_emb": dict(modulation=True, embedders=True),
}


def hf_vision(cfg, seed):
    from transformers import SiglipVisionConfig, SiglipVisionModel

    torch.manual_seed(seed)
    return SiglipVisionModel(SiglipVisionConfig(**cfg)).eval()


def native_siglip(hf, cfg, dev):
    from modules.image_embedders import SiglipVisionNative

    m = SiglipVisionNative(cfg)
    m.load_state_dict(hf.state_dict())
    return m.to(device=dev, dtype=torch.bfloat16)


def sample_images(n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        a = rng.integers(0, 256, (200 + 37 * i, 300 - 23 * i, 3), dtype=np.uint8)
        a[: a.shape[0] // 2] //= 2  # some structure: a darker upper half
        out.append(a)
    return out


def pixels(images):
    from modules.image_embedders import ReduxImageEncoder, SiglipVisionNative

    enc = ReduxImageEncoder(SiglipVisionNative(TINY), txt_in_features=16)
    return torch.cat([enc.preprocess(im) for im in images], 0)


# ---- 1. kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [729, 49, 37])
def test_vision_attention_padded_heads_vs_fp64(dev, L):
    from fluxmi import ops

    B, H, hd, hp = 2, 16, 72, 96
    Lp = (L + 31) // 32 * 32
    g = torch.Generator().manual_seed(L)
    q, k, v = (torch.randn(B, L, H, hd, generator=g).bfloat16() for _ in range(3))
    vb = (0.1 * torch.randn(H, hd, generator=g)).bfloat16()

    def pad(x):  # [B, L, H, hd] -> [B, Lp, H*hp], zero head columns and rows
        out = torch.zeros(B, Lp, H, hp, dtype=torch.bfloat16)
        out[:, :L, :, :hd] = x
        return out.reshape(B, Lp, H * hp)

    qk = torch.cat((pad(q), pad(k)), -1).to(dev)
    vt = pad(v).transpose(1, 2).contiguous().to(dev)  # [B, H*hp, Lp]
    vbp = torch.zeros(H, hp, dtype=torch.bfloat16)
    vbp[:, :hd] = vb
    scale = hd ** -0.5
    out = ops.vision_attention(qk[:, :, : H * hp], qk[:, :, H * hp:], vt, L, H, hp, scale, v_bias=vbp.reshape(-1).to(dev)).cpu()
    assert out.shape == (B, Lp, H * hp) and torch.isfinite(out).all()
    o = out.view(B, Lp, H, hp)
    assert (o[:, :, :, hd:] == 0).all(), "padded output columns must be zero"
    assert (o[:, L:] == 0).all(), "rows >= L are not written"
    s = torch.einsum("blhd,bmhd->bhlm", q.double(), k.double()) * scale
    ref = torch.einsum("bhlm,bmhd->blhd", torch.softmax(s, -1), v.double()) + vb.double()
    err = (o[:, :L, :, :hd].double() - ref).abs().max().item()
    print(f"vision attention L={L}: max |err| vs fp64 {err:.3e}")
    assert err <= 2e-2 * v.abs().max().item()


def test_vision_attention_at_64_equals_text_attention(dev):
    """head width 64 through the batched entry == fluxmi_text_attention per sequence, bit for bit (the same kernel)"""
    from fluxmi import ops

    B, H, L, Lp = 3, 4, 77, 96
    g = torch.Generator().manual_seed(0)
    qk = torch.randn(B, Lp, 2 * H * 64, generator=g).bfloat16().to(dev)
    vt = torch.randn(B, H * 64, Lp, generator=g).bfloat16().to(dev)
    vb = torch.randn(H * 64, generator=g).bfloat16().to(dev)
    got = ops.vision_attention(qk[:, :, : H * 64], qk[:, :, H * 64:], vt, L, H, 64, 0.125, v_bias=vb)
    for b in range(B):
        want = ops.text_attention(qk[b, :, : H * 64], qk[b, :, H * 64:], vt[b], L, H, scale=0.125, v_bias=vb)
        assert torch.equal(got[b, :L], want[:L])


def test_patch_embedding_vs_conv2d(dev):
    from fluxmi import _lib, ops

    B, D, P, G = 2, 1152, 14, 27
    g = torch.Generator().manual_seed(1)
    pix = (torch.rand(B, 3, 384, 384, generator=g) * 2 - 1).bfloat16()
    w = (torch.randn(D, 3, P, P, generator=g) / math.sqrt(588)).bfloat16()
    b = (0.1 * torch.randn(D, generator=g)).bfloat16()
    pos = (0.5 * torch.randn(G * G, D, generator=g)).bfloat16()
    patches = ops.patchify(pix.to(dev), P, G, 640)
    # the patch rows are the conv's im2col, bit for bit, with zero columns 588 .. 639; the unread border is pixels 378 .. 383
    cols = torch.nn.functional.unfold(pix.float(), P, stride=P).transpose(1, 2).reshape(B * G * G, 588)
    pc = patches.cpu()
    assert torch.equal(pc[:, :588].float(), cols) and (pc[:, 588:] == 0).all()
    w2 = torch.zeros(D, 640, dtype=torch.bfloat16)
    w2[:, :588] = w.reshape(D, 588)
    ones = torch.ones(D, dtype=torch.bfloat16, device=dev)
    resid = pos.repeat(B, 1).to(dev)
    got = ops.linear(patches, w2.to(dev), b.to(dev), epilogue=_lib.EPI_GATE_RESID, gate=ones, resid=resid, out=torch.empty_like(resid))
    ref = torch.nn.functional.conv2d(pix.float(), w.float(), b.float(), stride=P).flatten(2).transpose(1, 2) + pos.float()
    e = rel_l2(got.view(B, G * G, D), ref)
    print(f"patch embedding vs fp32 conv2d: rel-L2 {e:.3e}")
    assert e <= 4e-3


# ---- 2. SigLIP and the projector against transformers / fp32 ----------------------------------------------------------------------
def _siglip_gate(cfg, dev, seed, hf_bf16_dev):
    import copy

    hf = hf_vision(cfg, seed)
    pix = pixels(sample_images(2, seed))
    with torch.no_grad():
        ref = hf(pixel_values=pix).last_hidden_state.float()                                      # fp32 on the host
        hb = copy.deepcopy(hf).to(device=hf_bf16_dev, dtype=torch.bfloat16)
        yard = hb(pixel_values=pix.to(hf_bf16_dev, torch.bfloat16)).last_hidden_state.float().cpu()  # transformers in bf16
        del hb
    nat = native_siglip(hf, cfg, dev)
    got = nat(pix.to(dev))["last_hidden_state"]
    assert got.shape == ref.shape and got.dtype == torch.bfloat16 and torch.isfinite(got).all()
    d_nat, d_hf = rel_l2(got, ref), rel_l2(yard, ref)
    return nat, pix, d_nat, d_hf


def test_siglip_tiny_width_vs_transformers(dev):
    nat, pix, d_nat, d_hf = _siglip_gate(TINY, dev, 0, torch.device("cpu"))
    print(f"SigLIP hidden 144 / head 72 / 3 layers: native {d_nat:.3e} vs transformers bf16 {d_hf:.3e} (rel-L2 to fp32)")
    assert d_nat <= 1.5 * d_hf
    # batch invariance: image 1 alone == image 1 beside image 0
    one = nat(pix[1:].to(dev))["last_hidden_state"]
    both = nat(pix.to(dev))["last_hidden_state"]
    assert torch.equal(one[0], both[1])


def test_siglip_full_so400m_geometry_vs_transformers(dev):
    """27 x 1152 x 4304, 16 heads of 72, random weights; every GEMM it launches has a tiled config"""
    from fluxmi import ops
    from modules.image_embedders import SIGLIP_SO400M_384

    shapes = []
    orig = ops.gemm_grouped

    def record(groups, N, K, *a, **kw):
        shapes.append((N, K))
        return orig(groups, N, K, *a, **kw)

    nat, pix, d_nat, d_hf = None, None, None, None
    ops.gemm_grouped = record
    try:
        nat, pix, d_nat, d_hf = _siglip_gate(SIGLIP_SO400M_384, dev, 5, dev)
    finally:
        ops.gemm_grouped = orig
    print(f"SigLIP so400m: native {d_nat:.3e} vs transformers bf16 {d_hf:.3e} (rel-L2 to fp32)")
    assert d_nat <= 1.5 * d_hf
    want = {(1152, 640), (3072, 1152), (768, 1152), (1152, 1536), (4352, 1152), (1152, 4352)}
    assert set(shapes) == want, set(shapes) ^ want
    _assert_tiled(shapes, dev)


def _assert_tiled(shapes, dev):
    """each (N, K) runs on the 128 x 128 tile config when forced (the library refuses an untileable shape): the automatic choice then never
    falls back to the generic kernel (config 2 is one of its candidates)"""
    from fluxmi import ops

    for N, K in sorted(set(shapes)):
        a = torch.randn(64, K, device=dev).bfloat16()
        w = torch.randn(N, K, device=dev).bfloat16()
        ops.linear(a, w, tile_cfg=2)
        assert N % 128 == 0 and (2 * K) % 128 == 0
    torch.cuda.synchronize()


def test_redux_projector_vs_fp32(dev):
    from modules.image_embedders import ReduxImageEncoder, SiglipVisionNative
    from fluxmi import ops

    g = torch.Generator().manual_seed(2)
    sd = {"redux_up.weight": torch.randn(12288, 1152, generator=g) / math.sqrt(1152), "redux_up.bias": 0.02 * torch.randn(12288, generator=g),
          "redux_down.weight": torch.randn(4096, 12288, generator=g) / math.sqrt(12288), "redux_down.bias": 0.02 * torch.randn(4096, generator=g)}
    sd = {k: v.bfloat16() for k, v in sd.items()}
    enc = ReduxImageEncoder(SiglipVisionNative(dict(TINY, hidden_size=1152, num_attention_heads=16, num_hidden_layers=0)), txt_in_features=4096)
    enc.load_state_dict(sd)
    enc.to(dev)
    x = torch.randn(2, 729, 1152, generator=g).bfloat16()
    shapes = []
    orig = ops.gemm_grouped
    ops.gemm_grouped = lambda groups, N, K, *a, **kw: (shapes.append((N, K)), orig(groups, N, K, *a, **kw))[1]
    try:
        got = enc.project(x.to(dev))
    finally:
        ops.gemm_grouped = orig
    assert got.shape == (2, 729, 4096) and got.dtype == torch.bfloat16
    f = {k: v.float() for k, v in sd.items()}
    ref = torch.nn.functional.linear(torch.nn.functional.silu(torch.nn.functional.linear(x.float(), f["redux_up.weight"], f["redux_up.bias"])),
                                     f["redux_down.weight"], f["redux_down.bias"])
    b = {k: v.to(dev) for k, v in sd.items()}
    yard = torch.nn.functional.linear(torch.nn.functional.silu(torch.nn.functional.linear(x.to(dev), b["redux_up.weight"], b["redux_up.bias"])),
                                      b["redux_down.weight"], b["redux_down.bias"])
    d_nat, d_t = rel_l2(got, ref), rel_l2(yard, ref)
    print(f"Redux projector: native {d_nat:.3e} vs torch bf16 {d_t:.3e} (rel-L2 to fp32)")
    assert d_nat <= 1.5 * d_t
    assert set(shapes) == {(12288, 1152), (4096, 12288)}
    _assert_tiled(shapes, dev)


# ---- 3. the engine at odd text lengths --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qname", list(QUANTS))
@pytest.mark.parametrize("B", [1, 2])
def test_forward_at_odd_text_length_matches_oracle_through_calibration(dev, qname, B):
    from fluxmi import synth

    cfg = tiny_config()
    model, oracle, sd = build(cfg, QUANTS[qname], dev)
    oracle_bf16 = fo.FluxOracle({k: v.clone() for k, v in sd.items()}, fo.FluxParams(**cfg.params.model_dump()), quantize=None)
    inp = synth.make_inputs(cfg.params, 64, 80, 41, batch=B, seed=3, real_tokens=8)  # Lt 41, Li 20: L 61
    d = to_dev(inp, dev)
    worst = 0.0
    for step in range(15):
        t = torch.full((B,), 1.0 - 0.06 * step, dtype=torch.bfloat16)
        g = torch.full((B,), 3.5, dtype=torch.bfloat16)
        ref = oracle.forward(inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], t, inp["y"], g)
        got = model(d["img"], d["img_ids"], d["txt"], d["txt_ids"], t.to(dev), d["y"], g.to(dev))
        assert got.shape == inp["img"].shape and torch.isfinite(got).all()
        e = rel_l2(got, ref)
        worst = max(worst, e)
        if QUANTS[qname] is None:
            assert e <= 1e-2, f"{qname} call {step}: rel-L2 {e:.3e}"
        else:
            assert e <= 6e-2, f"{qname} call {step}: rel-L2 vs fp8 oracle {e:.3e}"
            if step in (0, 7, 14):
                rb = oracle_bf16.forward(inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], t, inp["y"], g)
                d_ref, d_got = rel_l2(ref, rb), rel_l2(got, rb)
                assert d_got <= 1.25 * d_ref, f"{qname} call {step}: vs bf16 flow {d_got:.3e} > 1.25 x {d_ref:.3e}"
    if QUANTS[qname] is not None:
        assert model.calibration_state()[0]
    print(f"[odd Lt 41, {qname}, B {B}] worst rel-L2 over 15 calls: {worst:.3e}")


def test_graph_denoise_equals_eager_at_odd_text_length(dev):
    from fluxmi import synth

    cfg = tiny_config()
    model, _, _ = build(cfg, QUANTS["fp8"], dev)
    d = to_dev(synth.make_inputs(cfg.params, 64, 64, 41, batch=2, seed=5, real_tokens=8), dev)
    ts = fo.get_schedule(16, d["img"].shape[1])
    run = lambda ts_, img, use_graph=True: model.denoise(img, d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts_, guidance=3.5,  # noqa: E731
                                                          use_graph=use_graph)
    lat = run(ts[:14], d["img"], use_graph=False)  # 13 calibrating steps
    assert model.calibration_state()[0]
    a, b = run(ts[:9], lat), run(ts[:9], lat, use_graph=False)
    assert torch.equal(a, b), f"graph vs eager at Lt 41: rel-L2 {rel_l2(a, b):.3e}"
    c = lat.clone()
    g = torch.full((2,), 3.5, dtype=torch.bfloat16, device=dev)
    for t_curr, t_prev in zip(ts[:9][:-1], ts[:9][1:]):
        tv = torch.full((2,), t_curr, dtype=torch.bfloat16, device=dev)
        c = c + (t_prev - t_curr) * model(c, d["img_ids"], d["txt"], d["txt_ids"], tv, d["y"], g, mode=1)
    assert torch.equal(a, c), f"graph loop vs python loop at Lt 41: rel-L2 {rel_l2(a, c):.3e}"


def test_schnell_bf16_at_odd_text_length(dev):
    from fluxmi import synth

    cfg = tiny_config(schnell=True)
    model, oracle, _ = build(cfg, None, dev)
    inp = synth.make_inputs(cfg.params, 64, 64, 37, batch=2, seed=9, real_tokens=8)
    d = to_dev(inp, dev)
    ts = fo.get_schedule(4, 16, shift=False)
    ref = fo.denoise(oracle, inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], ts, guidance=3.5)
    got = model.denoise(d["img"], d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts, guidance=3.5)
    e = rel_l2(got, ref)
    print(f"[schnell bf16, Lt 37] latents after 4 steps: rel-L2 {e:.3e}")
    assert e <= 1e-2


def test_headline_redux_shape_at_real_width(dev):
    """1024^2, Lt = 512 + 729 = 1241 (L = 5337), 1 + 1 blocks at hidden 3072: the bf16 flow's forward against the oracle, and the fp8 flow
    calibrated at this shape with its graph-replayed denoise equal to the eager one, bit for bit"""
    import util
    from fluxmi import synth

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    p = cfg.params
    p.depth, p.depth_single_blocks = 1, 1
    inp = synth.make_inputs(p, 1024, 1024, 1241, batch=1, seed=2, real_tokens=64)
    d = to_dev(inp, dev)
    assert d["txt"].shape[1] + d["img"].shape[1] == 5337
    model, oracle, _ = build(cfg, None, dev, seed=1)
    t = torch.full((1,), 0.5, dtype=torch.bfloat16)
    g = torch.full((1,), 3.5, dtype=torch.bfloat16)
    ref = oracle.forward(inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], t, inp["y"], g)
    got = model(d["img"], d["img_ids"], d["txt"], d["txt_ids"], t.to(dev), d["y"], g.to(dev))
    e = rel_l2(got, ref)
    print(f"[headline Redux L=5337, bf16] forward rel-L2 vs oracle {e:.3e}")
    assert torch.isfinite(got).all() and e <= 1e-2
    del model, oracle
    model, _, _ = build(cfg, QUANTS["fp8"], dev, seed=1)
    ts = fo.get_schedule(16, d["img"].shape[1])
    lat = model.denoise(d["img"], d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts[:14], guidance=3.5, use_graph=False)
    assert model.calibration_state()[0] and torch.isfinite(lat).all()
    a = model.denoise(lat, d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts[:5], guidance=3.5)
    b = model.denoise(lat, d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts[:5], guidance=3.5, use_graph=False)
    assert torch.isfinite(a).all() and torch.equal(a, b), f"graph vs eager at L = 5337: rel-L2 {rel_l2(a, b):.3e}"


# ---- 4. the pipeline end to end -----------------------------------------------------------------------------------------------------
def tiny_redux(dev, ctx=128, seed=0):
    from modules.image_embedders import ReduxImageEncoder

    hf = hf_vision(TINY, seed)
    enc = ReduxImageEncoder(native_siglip(hf, TINY, dev), txt_in_features=ctx)
    g = torch.Generator().manual_seed(seed + 1)
    enc.load_state_dict({"redux_up.weight": torch.randn(3 * ctx, 144, generator=g) / 12, "redux_up.bias": 0.02 * torch.randn(3 * ctx, generator=g),
                         "redux_down.weight": torch.randn(ctx, 3 * ctx, generator=g) / math.sqrt(3 * ctx),
                         "redux_down.bias": 0.02 * torch.randn(ctx, generator=g)})
    return enc.to(device=dev, dtype=torch.bfloat16)


def manual(pipe, prompt, images, seed, H, W, steps, num_images=1, **cond):
    """generate()'s request, composed by hand: same noise and schedule, txt = cat(T5 states, Redux tokens), txt_ids zeros"""
    generator, _ = pipe.set_seed(seed)
    noise, ts = pipe.preprocess_latent(height=H, width=W, num_steps=steps, generator=generator, num_images=num_images)
    img, img_ids, vec, txt, txt_ids = map(lambda x: x.contiguous(), pipe.prepare(noise, prompt))
    tok = pipe.redux(images).to(txt)
    tok = tok.reshape(1, -1, tok.shape[-1]).repeat(img.shape[0], 1, 1)
    txt = torch.cat((txt, tok), 1).contiguous()
    txt_ids = torch.zeros(txt.shape[0], txt.shape[1], 3, device=txt.device, dtype=txt.dtype)
    out = pipe.model.denoise(img, img_ids, txt, txt_ids, vec, ts, guidance=3.5, **cond)
    return pipe.unpack(out.float(), H, W), txt.shape[1]


def test_pipeline_redux_end_to_end(dev):
    import util
    from flux_pipeline import FluxPipeline
    from fluxmi import synth

    cfg = tiny_config()
    cfg.text_enc_max_length = 32
    pipe = FluxPipeline.load_pipeline_from_config(cfg, state_dict=synth.make_state_dict(cfg.params, seed=0))
    assert pipe.redux is None and util.load_redux(cfg) is None
    pipe.redux = tiny_redux(dev)
    pipe.compile()  # calibrates, then runs one Redux request
    g = torch.Generator().manual_seed(1)
    prompt = {"txt": 0.1 * torch.randn(1, 32, 128, generator=g), "vec": torch.randn(1, 64, generator=g)}
    a, b = sample_images(2, seed=3)
    kw = dict(width=64, height=96, num_steps=6, seed=7, silent=True, output_type="latent")
    lat = pipe.generate(prompt, redux_image=a, **kw)
    want, lt = manual(pipe, prompt, [a], 7, 96, 64, 6)
    assert lt == 32 + 729 and torch.equal(lat, want), f"generate vs manual composition: rel-L2 {rel_l2(lat, want):.3e}"
    plain = pipe.generate(prompt, **kw)
    assert not torch.equal(plain, lat)
    # a list of two images (Lt = 32 + 1458), two images per request
    two = pipe.generate(prompt, redux_image=[a, b], **kw)
    want2, lt2 = manual(pipe, prompt, [a, b], 7, 96, 64, 6)
    assert lt2 == 32 + 1458 and torch.equal(two, want2)
    n2 = pipe.generate(prompt, redux_image=a, **{**kw, "num_images": 2})
    assert n2.shape == (2,) + tuple(lat.shape[1:]) and torch.isfinite(n2).all()
    want3, _ = manual(pipe, prompt, [a], 7, 96, 64, 6, num_images=2)
    assert torch.equal(n2, want3)


def test_pipeline_fill_plus_redux(dev):
    from flux_pipeline import FluxPipeline
    from fluxmi import synth

    cfg = tiny_config()
    cfg.params.in_channels, cfg.params.out_channels = 384, 64
    cfg.text_enc_max_length = 32
    pipe = FluxPipeline.load_pipeline_from_config(cfg, state_dict=synth.make_state_dict(cfg.params, seed=2))
    pipe.redux = tiny_redux(dev, seed=4)
    pipe.compile()
    g = torch.Generator().manual_seed(3)
    prompt = {"txt": 0.1 * torch.randn(1, 32, 128, generator=g), "vec": torch.randn(1, 64, generator=g)}
    cond = torch.randn(1, 24, 320, generator=g).to(torch.bfloat16)  # Fill conditioning of a 64 x 96 image, prepared
    (a,) = sample_images(1, seed=5)
    kw = dict(width=64, height=96, num_steps=6, seed=11, silent=True, output_type="latent")
    lat = pipe.generate(prompt, redux_image=a, img_cond=cond, **kw)
    want, _ = manual(pipe, prompt, [a], 11, 96, 64, 6, img_cond=cond.to(dev))
    assert torch.equal(lat, want), f"Fill + Redux vs manual composition: rel-L2 {rel_l2(lat, want):.3e}"
    assert not torch.equal(lat, pipe.generate(prompt, img_cond=cond, **kw))
