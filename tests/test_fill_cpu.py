"""FLUX.1 Fill / Depth / Canny channel conditioning, host side: a Fill-shaped model loads, the conditioning packers against an independent
einops statement of BFL's expressions, the HTTP fields and the model's refusals.  No GPU."""
import io
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from einops import rearrange


def tiny_params(in_channels=384, out_channels=64):
    import util

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    p = cfg.params
    p.hidden_size, p.num_heads, p.depth, p.depth_single_blocks, p.context_in_dim, p.vec_in_dim = 256, 2, 1, 1, 128, 64
    p.in_channels, p.out_channels = in_channels, out_channels
    return cfg


@pytest.mark.parametrize("cin", [384, 128])
def test_fill_shaped_model_loads_with_the_dev_keys(cin):
    import dataclasses

    import flux_oracle as fo
    import util
    from fluxmi import synth

    cfg = tiny_params(cin, 64)
    sd = synth.make_state_dict(cfg.params, seed=0)
    assert sd["img_in.weight"].shape == (256, cin) and sd["final_layer.linear.weight"].shape == (64, 256)
    assert sd["final_layer.linear.bias"].shape == (64,)
    plain = tiny_params(64, None)
    sd_plain = synth.make_state_dict(plain.params, seed=0)
    assert set(sd) == set(sd_plain)
    model = util.load_flow_model(cfg, sd)
    assert model.in_channels == cin and model.out_channels == 64
    assert model.img_in.weight.shape == (256, cin) and model.final_layer.linear.weight.shape == (64, 256)
    assert torch.equal(model.img_in.weight, sd["img_in.weight"])
    # out_channels stays out of model_dump(): the oracle's dataclass takes exactly those fields
    assert set(cfg.params.model_dump()) == {f.name for f in dataclasses.fields(fo.FluxParams)}
    fo.FluxParams(**cfg.params.model_dump())
    # the inputs: noise of the 64 predicted channels
    inp = synth.make_inputs(cfg.params, 64, 64, 16, batch=2, seed=1)
    assert inp["img"].shape == (2, 16, 64)


def test_defaults_give_todays_tensors():
    from fluxmi import synth

    a = tiny_params(64, None).params
    b = tiny_params(64, 64).params
    sa, sb = synth.make_state_dict(a, seed=3), synth.make_state_dict(b, seed=3)
    assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    ia, ib = synth.make_inputs(a, 48, 80, 16, seed=2), synth.make_inputs(b, 48, 80, 16, seed=2)
    assert all(torch.equal(ia[k], ib[k]) for k in ia)
    assert a.model_dump() == b.model_dump()


def test_config_jsons_for_fill_and_depth():
    import os

    import util

    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flux-fp8-api_amd", "configs")
    for name, cin in (("fill", 384), ("depth", 128)):
        cfg = util.load_config_from_path(os.path.join(root, f"config-{name}-dev-mi355x.json"))
        assert cfg.version == "flux-dev" and cfg.params.in_channels == cin and cfg.params.out_channels == 64
        assert cfg.params.hidden_size == 3072 and "out_channels" not in cfg.params.model_dump()


def test_load_names_the_config_for_a_fill_checkpoint():
    import util
    from fluxmi import synth

    sd = synth.make_state_dict(tiny_params(384, 64).params, seed=0)
    with pytest.raises(ValueError, match="config-fill-dev-mi355x.json"):
        util.load_flow_model(tiny_params(64, None), sd)


def test_model_refuses_bad_channel_conditioning():
    """missing img_cond on a Fill model, img_cond on a plain model, a wrong width, img_cond with img_cond_seq: all before any device work"""
    import util
    from fluxmi import synth

    fill_cfg, plain_cfg = tiny_params(384, 64), tiny_params(64, None)
    fill = util.load_flow_model(fill_cfg, synth.make_state_dict(fill_cfg.params, seed=0))
    plain = util.load_flow_model(plain_cfg, synth.make_state_dict(plain_cfg.params, seed=0))
    inp = synth.make_inputs(fill_cfg.params, 32, 64, 8, batch=1, seed=0)
    img, ids, txt, tids, y = inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"]
    t, g = torch.ones(1), torch.full((1,), 3.5)
    good = torch.zeros(1, img.shape[1], 320)
    seq, seq_ids = torch.zeros(1, 3, 64), torch.zeros(1, 3, 3)
    fwd = lambda m, **kw: m(img, ids, txt, tids, t, y, g, **kw)
    den = lambda m, **kw: m.denoise(img, ids, txt, tids, y, [1.0, 0.0], **kw)
    for call in (fwd, den):
        with pytest.raises(ValueError, match="img_cond"):
            call(fill)
        with pytest.raises(ValueError, match="no conditioning channels"):
            call(plain, img_cond=good[..., :64])
        with pytest.raises(ValueError, match="img_cond"):
            call(fill, img_cond=good[..., :256])
        with pytest.raises(ValueError, match="img_cond"):
            call(fill, img_cond=good[:, :-1])
        with pytest.raises(ValueError, match="cannot be combined"):
            call(fill, img_cond=good, img_cond_seq=seq, img_cond_seq_ids=seq_ids)
    # what passes the checks is the channel concatenation, noisy channels first
    s = fill._with_channels(img, good + 1, None)
    assert s.shape == (1, img.shape[1], 384) and torch.equal(s[..., :64], img.bfloat16()) and (s[..., 64:] == 1).all()
    assert plain._with_channels(img, None, None) is img
    with pytest.raises(ValueError):
        util.load_flow_model(tiny_params(64, 128), None)  # out_channels > in_channels


# ---- the conditioning packers -----------------------------------------------------------------------------------------------------
class RecordingEncoder:
    """stands in for the autoencoder: records its input, returns a deterministic function of it ([1, 16, H/8, W/8])"""

    def __init__(self):
        self.inputs, self.noises = [], []
        self.encoder = SimpleNamespace(num_resolutions=4, conv_out=SimpleNamespace(out_channels=32))

    def encode(self, x, noise=None):
        self.inputs.append(x.clone())
        self.noises.append(noise.clone())
        b, _, H, W = x.shape
        z = torch.nn.functional.avg_pool2d(x.float(), 8)  # [1, 3, H/8, W/8]
        z = torch.cat([z * (k + 1) for k in range(6)], 1)[:, :16]
        return z + noise


def stub_pipeline():
    from flux_pipeline import FluxPipeline

    pipe = FluxPipeline.__new__(FluxPipeline)
    pipe.ae, pipe.ae_dtype, pipe.dtype = RecordingEncoder(), torch.float32, torch.bfloat16
    pipe.device_ae = pipe.device_flux = torch.device("cpu")
    return pipe


def bfl_fill(image_u8, mask_u8_l, z):
    """BFL's prepare_fill after the encode, restated with einops: z [1, 16, h, w] and the "L" mask -> [1, Li, 320]"""
    mask = torch.from_numpy(mask_u8_l).float() / 255.0
    mask = rearrange(mask, "h w -> 1 1 h w")[:, 0].to(torch.bfloat16)
    mask = rearrange(mask, "b (h ph) (w pw) -> b (ph pw) h w", ph=8, pw=8)
    mask = rearrange(mask, "b c (h ph) (w pw) -> b (h w) (c ph pw)", ph=2, pw=2)
    z = rearrange(z.to(torch.bfloat16), "b c (h ph) (w pw) -> b (h w) (c ph pw)", ph=2, pw=2)
    return torch.cat((z, mask), -1)


@pytest.mark.parametrize("binary", [False, True])
def test_fill_packers_match_bfl_expressions(binary):
    from PIL import Image

    from flux_pipeline import FluxPipeline

    H, W = 48, 80
    rng = np.random.default_rng(4 + binary)
    image = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    mask_rgb = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    if binary:
        mask_rgb = np.where(rng.random((H, W, 1)) < 0.3, 255, 0).astype(np.uint8).repeat(3, 2)
    mask_l = np.array(Image.fromarray(mask_rgb).convert("L"))
    # the mask packer alone: values and channel order
    m = torch.from_numpy(mask_l).float().div(255.0)[None, None]
    got = FluxPipeline.pack_fill_mask(m)
    want = bfl_fill(image, mask_l, torch.zeros(1, 16, H // 8, W // 8))[..., 64:]
    assert got.dtype == torch.bfloat16 and got.shape == (1, (H // 16) * (W // 16), 256) and torch.equal(got, want)
    # channel c = 4 * (8 * py + px) + 2 * qy + qx of token (i, j) is pixel (16 i + 8 qy + py, 16 j + 8 qx + px)
    i, j, py, px, qy, qx = 1, 3, 5, 2, 1, 0
    assert got[0, i * (W // 16) + j, 4 * (8 * py + px) + 2 * qy + qx] == m[0, 0, 16 * i + 8 * qy + py, 16 * j + 8 * qx + px].bfloat16()
    # the whole preparation through a recording encoder
    pipe = stub_pipeline()
    gen = torch.Generator().manual_seed(9)
    cond = pipe.prepare_fill_conditioning(image, mask_rgb, H, W, num_images=2, generator=gen)
    enc_in, eps = pipe.ae.inputs[-1], pipe.ae.noises[-1]
    x = torch.from_numpy(image).float().div(127.5).sub(1.0).permute(2, 0, 1)[None]
    assert torch.equal(enc_in, x * (1 - m)), "the encoder must see image * (1 - mask)"
    assert eps.shape == (1, 16, H // 8, W // 8)
    assert torch.equal(eps, torch.randn(1, 16, H // 8, W // 8, generator=torch.Generator().manual_seed(9)))
    z = pipe.ae.encode(x * (1 - m), noise=eps)
    want = bfl_fill(image, mask_l, z)
    assert cond.shape == (2, (H // 16) * (W // 16), 320) and cond.dtype == torch.bfloat16
    assert torch.equal(cond[0], want[0]) and torch.equal(cond[1], want[0])


def test_fill_resizes_only_when_the_size_differs():
    pipe = stub_pipeline()
    image = np.random.default_rng(0).integers(0, 256, size=(64, 96, 3), dtype=np.uint8)
    mask = np.zeros((64, 96), dtype=np.uint8)
    mask[:, 48:] = 255
    c = pipe.prepare_fill_conditioning(image, mask, 32, 48, generator=torch.Generator().manual_seed(0))
    assert c.shape == (1, 6, 320) and pipe.ae.inputs[-1].shape == (1, 3, 32, 48)
    m = c[0, :, 64:].float()
    assert (m.view(2, 3, 256)[:, 0] == 0).all() and (m.view(2, 3, 256)[:, 2] == 1).all()  # the mask's left / right halves survive


def test_control_packer_matches_bfl_expression():
    from PIL import Image

    pipe = stub_pipeline()
    rng = np.random.default_rng(1)
    ctl = rng.integers(0, 256, size=(40, 70, 3), dtype=np.uint8)
    cond = pipe.prepare_control_conditioning(Image.fromarray(ctl), 32, 64, num_images=3, generator=torch.Generator().manual_seed(2))
    x = torch.from_numpy(np.array(Image.fromarray(ctl).resize((64, 32), Image.LANCZOS))).float() / 127.5 - 1.0
    x = rearrange(x, "h w c -> 1 c h w")
    assert torch.equal(pipe.ae.inputs[-1], x)
    z = pipe.ae.encode(x, noise=pipe.ae.noises[-1])
    want = rearrange(z.to(torch.bfloat16), "b c (h ph) (w pw) -> b (h w) (c ph pw)", ph=2, pw=2)
    assert cond.shape == (3, 8, 64) and all(torch.equal(cond[k], want[0]) for k in range(3))


def test_http_mask_and_control_fields():
    """`mask_image` / `control_image` reach generate() only when set; a request without them produces exactly today's keyword arguments."""
    from fastapi.testclient import TestClient

    import api

    calls = []

    class Stub:
        def generate(self, **kw):
            calls.append(kw)
            return io.BytesIO(b"\xff\xd8jpeg-bytes\xff\xd9")

    api.app.state.model = Stub()
    c = TestClient(api.app)
    base = {"prompt": "a cat on a bench", "width": 512, "height": 512, "num_steps": 4, "seed": 7}
    assert c.post("/generate", json=base).status_code == 200
    assert set(calls[-1]) == {"prompt", "width", "height", "num_steps", "guidance", "seed", "strength", "init_image"}
    assert c.post("/generate", json={**base, "mask_image": None, "control_image": None}).status_code == 200
    assert "mask_image" not in calls[-1] and "control_image" not in calls[-1]
    r = c.post("/generate", json={**base, "init_image": "photo.png", "mask_image": "bWFzaw=="})
    assert r.status_code == 200 and r.content.startswith(b"\xff\xd8")
    assert calls[-1]["mask_image"] == "bWFzaw==" and calls[-1]["init_image"] == "photo.png" and "control_image" not in calls[-1]
    r = c.post("/generate", json={**base, "control_image": "depth.png"})
    assert r.status_code == 200 and calls[-1]["control_image"] == "depth.png" and "mask_image" not in calls[-1]
