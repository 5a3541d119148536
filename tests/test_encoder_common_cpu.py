"""What the native towers share (modules/encoder_common.py), host side: the padded layer weights of the CLIP vision and CLIP text models (the
SigLIP case is tests/test_redux_cpu.py::test_padded_weights_unpad_to_the_originals), the weight cache on a value that is no tensor, and the
image normaliser against the three formulas the preprocessors used to spell out.  No GPU."""
import numpy as np
import torch
from torch import nn


def randomise(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
    return m


def bf(t):
    return t.detach().to(torch.bfloat16)


def test_clip_vision_padded_weights_unpad_to_the_originals():
    from modules.image_embedders import ClipVisionNative, unpad_heads

    # heads of 48 run at width 64; fc1 / fc2 of 200 pad to 256
    m = randomise(ClipVisionNative(dict(hidden_size=96, intermediate_size=200, num_hidden_layers=2, num_attention_heads=2, image_size=28,
                                        patch_size=14, projection_dim=32)), 1)
    H, hd, hp, D, F, Fp = 2, m.head_dim, m.head_pad, 96, 200, m.mlp_pad
    assert (hd, hp, Fp) == (48, 64, 256)
    lay = m.vision_model.encoder.layers[1]
    sa, mlp = lay.self_attn, lay.mlp
    p = m.padded_weights(1)
    assert sorted(p) == sorted("wqk bqk wv bv wo bo w1 b1 w2 b2 g1 e1 g2 e2".split())
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
    for name, src in (("bo", sa.out_proj.bias), ("b2", mlp.fc2.bias), ("g1", lay.layer_norm1.weight), ("e1", lay.layer_norm1.bias),
                      ("g2", lay.layer_norm2.weight), ("e2", lay.layer_norm2.bias)):
        assert torch.equal(p[name], bf(src)), name
    again = m.padded_weights(1)
    assert all(again[k] is p[k] for k in p), "padded weights are built once"


def test_clip_text_weights_are_the_bf16_originals():
    from modules.conditioner import ClipTextNative

    m = randomise(ClipTextNative(dict(vocab_size=40, hidden_size=128, num_attention_heads=2, intermediate_size=200, num_hidden_layers=2)), 2)
    lay = m.text_model.encoder.layers[1]
    sa, mlp = lay.self_attn, lay.mlp
    p = m.padded_weights(1)
    assert sorted(p) == sorted("wqk bqk wv bv wo bo w1 b1 w2 b2 g1 e1 g2 e2".split())
    assert torch.equal(p["wqk"], torch.cat([bf(sa.q_proj.weight), bf(sa.k_proj.weight)], 0))
    assert torch.equal(p["bqk"], torch.cat([bf(sa.q_proj.bias), bf(sa.k_proj.bias)], 0))
    for name, src in (("wv", sa.v_proj.weight), ("bv", sa.v_proj.bias), ("wo", sa.out_proj.weight), ("bo", sa.out_proj.bias),
                      ("w1", mlp.fc1.weight), ("b1", mlp.fc1.bias), ("w2", mlp.fc2.weight), ("b2", mlp.fc2.bias),
                      ("g1", lay.layer_norm1.weight), ("e1", lay.layer_norm1.bias), ("g2", lay.layer_norm2.weight), ("e2", lay.layer_norm2.bias)):
        assert p[name].dtype == torch.bfloat16 and p[name].is_contiguous() and torch.equal(p[name], bf(src)), name
    again = m.padded_weights(1)
    assert all(again[k] is p[k] for k in p), "the weights are prepared once"


def test_cache_holds_a_dict_and_keeps_its_rebuild_rule():
    from modules.conditioner import _Cache

    ck, builds = _Cache(), []
    a, b = nn.Parameter(torch.ones(3), requires_grad=False), nn.Parameter(torch.zeros(3), requires_grad=False)

    def build():
        builds.append(1)
        return {"sum": a.detach() + b.detach(), "n": len(builds)}

    v = ck.get("k", [a, b], build)
    assert v["n"] == 1 and ck.get("k", [a, b], build) is v and len(builds) == 1, "built once"
    b = b2 = nn.Parameter(torch.full((3,), 2.0), requires_grad=False)
    v2 = ck.get("k", [a, b2], build)
    assert v2["n"] == 2 and v2 is not v and torch.equal(v2["sum"], torch.full((3,), 3.0)), "rebuilt after a source parameter is replaced"
    assert ck.get("k", [a, b2], build) is v2
    assert ck.get("other", [a], lambda: "a string") == "a string"
    # Module.to(device) keeps the parameter objects and moves their data, so the sources' device changes under the same objects.  torch
    # refuses to move a host parameter's data to `meta` in place, so the source here is a stand-in that has what _Cache reads: `.device`
    src = type("Source", (), {"device": torch.device("cpu")})()
    w = ck.get("moved", [src], lambda: {"n": 1})
    assert ck.get("moved", [src], lambda: {"n": 2}) is w
    src.device = torch.empty(0, device="meta").device
    w2 = ck.get("moved", [src], lambda: {"n": 2})
    assert w2["n"] == 2 and ck.get("moved", [src], lambda: {"n": 3}) is w2, "rebuilt once after the sources moved to another device"


def test_normalize_image_equals_the_three_preprocessors_formulas():
    from modules.depth import IMAGENET_MEAN, IMAGENET_STD
    from modules.encoder_common import normalize_image
    from modules.ip_adapter import CLIP_MEAN, CLIP_STD

    img = np.random.default_rng(5).integers(0, 256, size=(13, 7, 3), dtype=np.uint8)
    img[0, 0], img[0, 1] = 0, 255
    chw = lambda a: torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))[None]  # noqa: E731
    # ReduxImageEncoder.preprocess (SiglipImageProcessor)
    a = (img.astype(np.float64) * (1 / 255)).astype(np.float32)
    redux = chw((a - np.float32(0.5)) / np.float32(0.5))
    got = normalize_image(img, np.float32(0.5), np.float32(0.5))
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, 13, 7) and got.is_contiguous()
    assert torch.equal(got.view(torch.int32), redux.view(torch.int32))
    # DepthAnythingNative.preprocess (DPTImageProcessor) and ip_adapter.clip_preprocess (CLIPImageProcessor)
    for mean, std in ((IMAGENET_MEAN, IMAGENET_STD), (CLIP_MEAN, CLIP_STD)):
        a = (img.astype(np.float64) * (1 / 255)).astype(np.float32)
        want = chw((a - np.array(mean, dtype=np.float32)) / np.array(std, dtype=np.float32))
        got = normalize_image(img, mean, std)
        assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32))
