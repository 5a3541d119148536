"""FLUX.1 Redux, host side: SigLIP preprocessing against transformers, checkpoint loading and the load-time padding of the native SigLIP,
token assembly against BFL's expressions on a stub encoder, the loader / config / HTTP surface.  No GPU."""
import base64
import io
import json
import os

import numpy as np
import pytest
import torch
from einops import repeat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(hidden_size=144, intermediate_size=344, num_hidden_layers=3, num_attention_heads=2, image_size=384, patch_size=14,
            num_channels=3, hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-6)


def tiny_siglip():
    from modules.image_embedders import SiglipVisionNative

    return SiglipVisionNative(TINY)


def hf_vision(seed=0, **over):
    from transformers import SiglipVisionConfig, SiglipVisionModel

    torch.manual_seed(seed)
    return SiglipVisionModel(SiglipVisionConfig(**{**TINY, **over})).eval()


# ---- 1. preprocessing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,mode", [((500, 333), "RGB"), ((97, 211), "RGBA"), ((384, 384), "L"), ((1023, 769), "RGB"), ((13, 7), "RGBA")])
def test_preprocess_matches_transformers(size, mode):
    from PIL import Image
    from transformers import SiglipImageProcessorPil

    from modules.image_embedders import ReduxImageEncoder

    enc = ReduxImageEncoder(tiny_siglip(), txt_in_features=16)
    proc = SiglipImageProcessorPil(size={"height": 384, "width": 384})
    w, h = size
    ch = {"RGB": 3, "RGBA": 4, "L": 1}[mode]
    arr = np.random.default_rng(w * h).integers(0, 256, (h, w, ch), dtype=np.uint8)
    arr = arr[..., 0] if mode == "L" else arr
    img = Image.fromarray(arr, mode)
    want = proc(images=[img], return_tensors="pt")["pixel_values"]
    got = enc.preprocess(img)
    assert got.dtype == torch.float32 and got.shape == (1, 3, 384, 384)
    assert torch.equal(got, want)
    # every input form gives the same tensor: ndarray, uint8 tensor, file path, base64 and data-URL of a PNG
    buf = io.BytesIO()
    img.save(buf, format="PNG")
    b64 = base64.b64encode(buf.getvalue()).decode()
    forms = [arr, torch.from_numpy(arr), b64, "data:image/png;base64," + b64]
    for f in forms:
        assert torch.equal(enc.preprocess(f), want), type(f).__name__


def test_preprocess_from_a_path(tmp_path):
    from PIL import Image
    from transformers import SiglipImageProcessorPil

    from modules.image_embedders import ReduxImageEncoder

    arr = np.random.default_rng(1).integers(0, 256, (120, 90, 3), dtype=np.uint8)
    p = tmp_path / "x.png"
    Image.fromarray(arr).save(p)
    want = SiglipImageProcessorPil(size={"height": 384, "width": 384})(images=[Image.open(p)], return_tensors="pt")["pixel_values"]
    assert torch.equal(ReduxImageEncoder(tiny_siglip(), txt_in_features=16).preprocess(str(p)), want)
    with pytest.raises(TypeError):
        ReduxImageEncoder(tiny_siglip(), txt_in_features=16).preprocess(arr.astype(np.float32))


# ---- 2. loading and padding ---------------------------------------------------------------------------------------------------------
def test_siglip_loads_transformers_keys_and_a_full_siglip_model():
    from transformers import SiglipConfig, SiglipModel

    hf = hf_vision()
    sd = hf.state_dict()
    m = tiny_siglip()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not missing and not unexpected
    msd = m.state_dict()
    for k, v in sd.items():
        if not k.startswith("head."):
            assert torch.equal(msd[k if k.startswith("vision_model.") else "vision_model." + k], v), k
    # a full SiglipModel checkpoint: the text tower, logit_scale / logit_bias and the pooling head are ignored
    torch.manual_seed(1)
    full = SiglipModel(SiglipConfig(vision_config=TINY, text_config=dict(hidden_size=32, intermediate_size=64, num_hidden_layers=1,
                                                                        num_attention_heads=2, vocab_size=100)))
    fsd = full.state_dict()
    assert any(k.startswith("text_model.") for k in fsd) and any(k.startswith("vision_model.head.") for k in fsd) and "logit_scale" in fsd
    m2 = tiny_siglip()
    m2.load_state_dict(fsd, strict=True)
    assert torch.equal(m2.vision_model.post_layernorm.weight, fsd["vision_model.post_layernorm.weight"])
    # the nested config of a SiglipModel config.json selects the vision tower
    from modules.image_embedders import SiglipVisionNative

    assert SiglipVisionNative({"vision_config": TINY}).cfg["hidden_size"] == 144
    # missing keys raise
    bad = {k: v for k, v in sd.items() if "layers.1.mlp.fc2" not in k}
    with pytest.raises(RuntimeError, match="fc2"):
        tiny_siglip().load_state_dict(bad, strict=True)


def test_read_siglip_from_a_directory(tmp_path):
    from safetensors.torch import save_file

    from modules.image_embedders import read_siglip

    hf = hf_vision(seed=2)
    d = tmp_path / "siglip"
    d.mkdir()
    (d / "config.json").write_text(json.dumps({"model_type": "siglip_vision_model", **TINY}))
    save_file({k: v.contiguous() for k, v in hf.state_dict().items()}, str(d / "model.safetensors"))
    m = read_siglip(str(d))
    assert m.cfg["num_hidden_layers"] == 3 and m.head_dim == 72 and m.head_pad == 96
    assert torch.equal(m.vision_model.encoder.layers[2].mlp.fc1.weight, hf.state_dict()["encoder.layers.2.mlp.fc1.weight"])
    save_file({k: v.contiguous() for k, v in hf.state_dict().items() if "post_layernorm" not in k}, str(d / "model.safetensors"))
    with pytest.raises(RuntimeError, match="missing"):
        read_siglip(str(d))


@pytest.mark.parametrize("geometry", ["tiny", "so400m"])
def test_padded_weights_unpad_to_the_originals(geometry):
    from modules.image_embedders import SiglipVisionNative, unpad_heads

    if geometry == "tiny":
        m = tiny_siglip()
        m.load_state_dict(hf_vision(seed=3).state_dict())
    else:
        m = SiglipVisionNative(None)  # so400m-patch14-384, default-initialised weights (only the shapes and the padding matter here)
        m.vision_model.encoder.layers = m.vision_model.encoder.layers[:1]
    H, hd, hp, D = m.cfg["num_attention_heads"], m.head_dim, m.head_pad, m.cfg["hidden_size"]
    F, Fp = m.cfg["intermediate_size"], m.mlp_pad
    assert hd == 72 and hp == 96 and Fp % 256 == 0 and Fp - F < 256 and m.seq_pad % 256 == 0 and m.patch_k % 64 == 0
    if geometry == "so400m":
        assert (D, F, Fp, m.seq_pad, m.patch_k, m.num_tokens) == (1152, 4304, 4352, 768, 640, 729)
    lay = m.vision_model.encoder.layers[0]
    sa, mlp = lay.self_attn, lay.mlp
    p = m.padded_weights(0)
    bf = lambda t: t.detach().to(torch.bfloat16)  # noqa: E731
    assert p["wqk"].shape == (2 * H * hp, D) and p["wv"].shape == (H * hp, D) and p["wo"].shape == (D, H * hp)
    assert p["w1"].shape == (Fp, D) and p["b1"].shape == (Fp,) and p["w2"].shape == (D, Fp)
    wq, wk = p["wqk"][: H * hp], p["wqk"][H * hp:]
    bq, bk = p["bqk"][: H * hp], p["bqk"][H * hp:]
    for got, src in ((wq, sa.q_proj.weight), (wk, sa.k_proj.weight), (p["wv"], sa.v_proj.weight), (bq, sa.q_proj.bias), (bk, sa.k_proj.bias),
                     (p["bv"], sa.v_proj.bias)):
        assert torch.equal(unpad_heads(got, H, hd, hp), bf(src))
        assert (got.reshape(H, hp, -1)[:, hd:] == 0).all()
    assert torch.equal(unpad_heads(p["wo"], H, hd, hp, dim=1), bf(sa.out_proj.weight))
    assert (p["wo"].reshape(D, H, hp)[:, :, hd:] == 0).all()
    assert torch.equal(p["w1"][:F], bf(mlp.fc1.weight)) and (p["w1"][F:] == 0).all()
    assert torch.equal(p["b1"][:F], bf(mlp.fc1.bias)) and (p["b1"][F:] == 0).all()
    assert torch.equal(p["w2"][:, :F], bf(mlp.fc2.weight)) and (p["w2"][:, F:] == 0).all()
    e = m.padded_weights("embed")
    kc = 3 * m.cfg["patch_size"] ** 2
    pe = m.vision_model.embeddings.patch_embedding.weight
    assert torch.equal(e["w"][:, :kc], bf(pe).reshape(D, kc)) and (e["w"][:, kc:] == 0).all()
    assert m.padded_weights(0)["wqk"] is p["wqk"], "padded weights are built once"


def test_redux_projector_loads_bfl_keys():
    from modules.image_embedders import ReduxImageEncoder

    g = torch.Generator().manual_seed(0)
    sd = {"redux_up.weight": torch.randn(48, 144, generator=g), "redux_up.bias": torch.randn(48, generator=g),
          "redux_down.weight": torch.randn(16, 48, generator=g), "redux_down.bias": torch.randn(16, generator=g)}
    enc = ReduxImageEncoder(tiny_siglip(), txt_in_features=16)
    enc.load_state_dict(sd)
    assert all(torch.equal(enc.state_dict()[k], v) for k, v in sd.items())
    assert enc.num_tokens == 729
    with pytest.raises(RuntimeError, match="redux_down.bias"):
        ReduxImageEncoder(tiny_siglip(), txt_in_features=16).load_state_dict({k: v for k, v in sd.items() if k != "redux_down.bias"})


# ---- 3. token assembly ------------------------------------------------------------------------------------------------------------
class StubRedux:
    """stands in for ReduxImageEncoder: T tokens of width C per image, a deterministic function of the image"""

    def __init__(self, T=5, C=16):
        self.num_tokens, self.C, self.calls = T, C, []

    def __call__(self, images):
        self.calls.append(len(images))
        out = []
        for im in images:
            a = torch.from_numpy(np.asarray(im, dtype=np.float32)).mean()
            out.append(a + torch.arange(self.num_tokens * self.C, dtype=torch.float32).view(1, self.num_tokens, self.C) / 7)
        return torch.cat(out, 0).to(torch.bfloat16)


def stub_pipeline(redux):
    from flux_pipeline import FluxPipeline

    pipe = FluxPipeline.__new__(FluxPipeline)
    pipe.redux, pipe.dtype = redux, torch.bfloat16
    pipe.device_ae = pipe.device_flux = torch.device("cpu")
    return pipe


def bfl_redux(t5, img_cond, bs):
    """BFL's prepare_redux after the encoder, restated: repeat txt and img_cond over the batch, cat on the token axis, zero txt_ids"""
    txt = repeat(t5, "1 ... -> bs ...", bs=bs) if t5.shape[0] == 1 and bs > 1 else t5
    img_cond = img_cond.to(torch.bfloat16)
    if img_cond.shape[0] == 1 and bs > 1:
        img_cond = repeat(img_cond, "1 ... -> bs ...", bs=bs)
    txt = torch.cat((txt, img_cond.to(txt)), dim=-2)
    return txt, torch.zeros(bs, txt.shape[1], 3)


@pytest.mark.parametrize("bs", [1, 3])
def test_token_assembly_matches_bfl(bs):
    rng = np.random.default_rng(2)
    a, b = (rng.integers(0, 256, (32, 48, 3), dtype=np.uint8) for _ in range(2))
    stub = StubRedux()
    pipe = stub_pipeline(stub)
    t5 = torch.randn(1, 8, 16, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16).repeat(bs, 1, 1)
    txt, ids = pipe.prepare_redux_tokens(a, num_images=bs, txt=t5)
    want, want_ids = bfl_redux(t5[:1], stub([a]), bs)
    assert txt.shape == (bs, 8 + 5, 16) and torch.equal(txt, want) and torch.equal(ids, want_ids.to(ids))
    assert ids.dtype == txt.dtype and (ids == 0).all()
    # a list of two: the second image's tokens follow the first's (Lt = Lt5 + 2 T)
    txt2, ids2 = pipe.prepare_redux_tokens([a, b], num_images=bs, txt=t5)
    tok = stub([a, b])
    want2, _ = bfl_redux(t5[:1], torch.cat((tok[:1], tok[1:]), 1), bs)
    assert txt2.shape == (bs, 8 + 10, 16) and torch.equal(txt2, want2) and ids2.shape == (bs, 18, 3)
    assert not torch.equal(txt2[:, 8:13], txt2[:, 13:18])
    # tokens alone
    only = pipe.prepare_redux_tokens([b], num_images=bs)
    assert only.shape == (bs, 5, 16) and torch.equal(only, repeat(stub([b]), "1 ... -> n ...", n=bs))


def test_redux_without_an_encoder_raises():
    pipe = stub_pipeline(None)
    with pytest.raises(ValueError, match="redux_path.*siglip_path"):
        pipe.generate({"txt": torch.zeros(1, 8, 16), "vec": torch.zeros(1, 8)}, redux_image=np.zeros((8, 8, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="redux_path"):
        pipe.prepare_redux_tokens(np.zeros((8, 8, 3), dtype=np.uint8))


# ---- 4. loader, config, HTTP ------------------------------------------------------------------------------------------------------
def test_load_redux_offline_and_from_local_files(tmp_path):
    from safetensors.torch import save_file

    import util

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    assert cfg.redux_path is None and cfg.siglip_path is None
    assert util.load_redux(cfg) is None
    cfg.redux_path, cfg.siglip_path = "/nonexistent/flux1-redux-dev.safetensors", "/nonexistent/siglip"
    assert util.load_redux(cfg) is None
    # local files: a tiny SigLIP directory and a BFL-keyed projector of width 16
    d = tmp_path / "siglip"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(TINY))
    save_file({k: v.contiguous() for k, v in hf_vision(seed=4).state_dict().items()}, str(d / "model.safetensors"))
    g = torch.Generator().manual_seed(0)
    red = {"redux_up.weight": torch.randn(48, 144, generator=g), "redux_up.bias": torch.randn(48, generator=g),
           "redux_down.weight": torch.randn(16, 48, generator=g), "redux_down.bias": torch.randn(16, generator=g)}
    save_file(red, str(tmp_path / "redux.safetensors"))
    cfg.redux_path = str(tmp_path / "redux.safetensors")
    assert util.load_redux(cfg) is None  # the SigLIP path still missing
    cfg.siglip_path, cfg.text_enc_device = str(d), "cpu"
    enc = util.load_redux(cfg)
    assert enc is not None and enc.redux_down.weight.shape == (16, 48) and enc.redux_down.weight.dtype == torch.bfloat16
    assert torch.equal(enc.redux_up.bias, red["redux_up.bias"].to(torch.bfloat16))


def test_redux_config_json_loads():
    import util

    base = util.load_config_from_path(os.path.join(ROOT, "flux-fp8-api_amd", "configs", "config-dev-mi355x.json"))
    cfg = util.load_config_from_path(os.path.join(ROOT, "flux-fp8-api_amd", "configs", "config-dev-redux-mi355x.json"))
    assert cfg.params.hidden_size == 3072 and cfg.version == "flux-dev"
    assert cfg.redux_path.endswith("flux1-redux-dev.safetensors") and cfg.siglip_path
    d0, d1 = base.model_dump(), cfg.model_dump()
    assert {k for k in d1 if d1[k] != d0[k]} == {"redux_path", "siglip_path"}
    assert util.load_redux(cfg) is None  # the shipped names are not local files here


def test_http_redux_field():
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
    assert c.post("/generate", json={**base, "redux_image": None}).status_code == 200
    assert "redux_image" not in calls[-1]
    r = c.post("/generate", json={**base, "redux_image": "c3R5bGU=", "mask_image": "bWFzaw==", "init_image": "a.png"})
    assert r.status_code == 200 and calls[-1]["redux_image"] == "c3R5bGU=" and calls[-1]["mask_image"] == "bWFzaw=="
