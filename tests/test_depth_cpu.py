"""The Depth Anything estimator, the parts that need no GPU: tests/depth_ref.py equals transformers' DepthAnythingForDepthEstimation in
fp64, DepthAnythingNative loads that state dict strict and refuses by name what it does not cover, its channel padding is exact, the
position-embedding interpolation and the input-size rule are transformers', the depth -> map reference behaves as include/fluxmi.h says,
the synthetic weights give a depth worth comparing, and the pipeline and the HTTP API refuse bad requests before any work."""
import io
import json

import numpy as np
import pytest
import torch

import depth_ref as dr

SEED = 0


@pytest.fixture(scope="module")
def tiny():
    """(config dict, synthetic state dict fp32, the transformers model in fp64 on it)"""
    from fluxmi import synth

    cfg = dr.tiny_config()
    sd = synth.make_depth_anything_state_dict(cfg, SEED)
    hf = dr.hf_model(cfg)
    hf.load_state_dict(sd, strict=True)
    return cfg, sd, hf.double()


@pytest.fixture(scope="module")
def ref_depths(tiny):
    """the fp64 reference depth of every grid, B = 2, computed once"""
    cfg, sd, _ = tiny
    sd64 = {k: v.double() for k, v in sd.items()}
    return {g: dr.forward(sd64, cfg, dr.pixel_values(2, *g)) for g in dr.GRIDS}


@pytest.mark.parametrize("grid", dr.GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_reference_equals_transformers_in_fp64(tiny, ref_depths, grid):
    cfg, sd, hf = tiny
    pix = dr.pixel_values(2, *grid)
    with torch.no_grad():
        want = hf(pix.double()).predicted_depth
    got = ref_depths[grid]
    assert got.shape == want.shape == (2, 14 * grid[0], 14 * grid[1])
    e = dr.rel_l2(got, want)
    print(f"depth_ref fp64 vs transformers fp64 at {grid}: rel-L2 {e:.3e}")
    assert e <= 1e-9


@pytest.mark.parametrize("grid", dr.GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_synthetic_weights_give_a_depth_worth_comparing(ref_depths, grid):
    """transformers' own init ends in ~4e-5 that the last ReLU mostly zeroes; the synthetic one must not"""
    d = ref_depths[grid]
    for b in range(d.shape[0]):
        assert float((d[b] > 0).double().mean()) >= 0.9
        assert float(d[b].max() - d[b].min()) >= 0.1 * float(d[b].max()) > 0
    assert not torch.equal(d[0], d[1])


def test_bf16_rounding_points_stay_close_and_differ(tiny, ref_depths):
    cfg, sd, _ = tiny
    g = (3, 5)
    rb = dr.forward(sd, cfg, dr.pixel_values(2, *g), torch.bfloat16)
    e = dr.rel_l2(rb, ref_depths[g])
    assert 1e-5 < e < 3e-2, e


# ---- loading ---------------------------------------------------------------------------------------------------------------------------------
def test_native_loads_the_transformers_state_dict_strict(tiny, tmp_path):
    from safetensors.torch import save_file

    import util
    from modules.depth import DepthAnythingNative, read_depth_anything

    cfg, sd, hf = tiny
    nat = DepthAnythingNative(cfg)
    hf_sd = {k: v.float() for k, v in hf.state_dict().items()}
    assert "backbone.embeddings.mask_token" in hf_sd
    res = nat.load_state_dict(hf_sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert set(nat.state_dict()) == set(hf_sd) - {"backbone.embeddings.mask_token"}
    with pytest.raises(RuntimeError, match="Unexpected key"):
        nat.load_state_dict({**hf_sd, "head.conv4.weight": torch.zeros(1)}, strict=True)
    with pytest.raises(RuntimeError, match="Missing key"):
        nat.load_state_dict({k: v for k, v in hf_sd.items() if k != "head.conv3.bias"}, strict=True)
    with pytest.raises(RuntimeError, match="GPU"):
        nat(dr.pixel_values(1, 1, 1))
    # a local directory: config.json + model.safetensors, or a .bin; the pipeline's loader returns None without one
    d = tmp_path / "depth-anything-tiny"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(cfg))
    save_file({k: v.contiguous() for k, v in hf_sd.items()}, str(d / "model.safetensors"))
    m = read_depth_anything(str(d))
    assert all(torch.equal(v, hf_sd[k]) for k, v in m.state_dict().items())
    b = tmp_path / "depth-anything-bin"
    b.mkdir()
    (b / "config.json").write_text(json.dumps(cfg))
    torch.save(hf_sd, str(b / "pytorch_model.bin"))
    assert all(torch.equal(v, hf_sd[k]) for k, v in read_depth_anything(str(b)).state_dict().items())
    spec = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    assert util.ModelSpec.model_fields["depth_path"].default is None and util.load_depth_model(spec, device="cpu") is None
    spec.depth_path = str(tmp_path / "missing")
    assert util.load_depth_model(spec, device="cpu") is None
    spec.depth_path = str(d)
    loaded = util.load_depth_model(spec, device="cpu")
    assert isinstance(loaded, DepthAnythingNative) and loaded.head.conv3.weight.dtype == torch.bfloat16
    with pytest.raises(FileNotFoundError, match="config.json"):
        read_depth_anything(str(tmp_path))


def test_config_defaults_are_read_as_transformers_reads_them():
    from transformers import DepthAnythingConfig, Dinov2Config

    from modules.depth import resolve_config

    c = resolve_config({"backbone_config": {"model_type": "dinov2", "hidden_size": 384, "num_attention_heads": 6, "out_indices": [9, 10, 11, 12],
                                            "reshape_hidden_states": False}})
    want, wb = DepthAnythingConfig(), Dinov2Config()
    same = lambda a, b: (list(a) == list(b)) if isinstance(a, (list, tuple)) else a == b  # noqa: E731  (a tuple here, a list from JSON)
    for k in ("reassemble_factors", "neck_hidden_sizes", "fusion_hidden_size", "head_hidden_size", "head_in_index", "depth_estimation_type"):
        assert same(c[k], getattr(want, k)), k
    for k in ("num_hidden_layers", "mlp_ratio", "layer_norm_eps", "hidden_act", "qkv_bias", "apply_layernorm", "use_swiglu_ffn", "patch_size"):
        assert c["backbone_config"][k] == getattr(wb, k), k
    assert wb.reshape_hidden_states is True  # the backbone's own default, which Depth Anything's checkpoints override
    # no backbone_config at all: DepthAnythingConfig's default DINOv2 small
    d = resolve_config({})["backbone_config"]
    for k in ("hidden_size", "num_attention_heads", "image_size", "out_indices", "reshape_hidden_states", "apply_layernorm"):
        assert same(d[k], getattr(want.backbone_config, k)), k
    # out_features name the same layers
    f = resolve_config({"backbone_config": {"hidden_size": 384, "num_attention_heads": 6, "out_features": ["stage3", "stage6", "stage9", "stage12"],
                                            "reshape_hidden_states": False}})
    assert f["backbone_config"]["out_indices"] == [3, 6, 9, 12]


@pytest.mark.parametrize("change,match", [
    (dict(depth_estimation_type="metric"), "depth_estimation_type='metric'"),
    (dict(use_swiglu_ffn=True), "use_swiglu_ffn"),
    (dict(model_type="beit"), "DINOv2 backbone"),
    (dict(hidden_act="gelu_pytorch_tanh"), "hidden_act"),
    (dict(reshape_hidden_states=True), "reshape_hidden_states"),
    (dict(head_hidden_size=128), "head_hidden_size=128"),
], ids=lambda v: v if isinstance(v, str) else "")
def test_native_refuses_by_name(change, match):
    from modules.depth import DepthAnythingNative

    with pytest.raises(ValueError, match=match):
        DepthAnythingNative(dr.tiny_config(**change))
    with pytest.raises(ValueError, match="backbone="):
        DepthAnythingNative({"backbone": "facebook/dinov2-small"})


# ---- padding ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over", [dict(), dict(head_hidden_size=96, neck_hidden_sizes=[48, 96, 192, 384])], ids=["tiny", "ragged_widths"])
def test_padded_weights_are_exact(over):
    """the channel-padded model the decoder kernels run: its pads are zeros around the checkpoint's own bits, it has the shapes the kernels'
    rules ask for, and tests/depth_ref.py computes the same depth from it -- bit for bit under the native rounding points, and to fp64
    summation order without rounding (a longer sum of the same terms and exact zeros may be blocked differently)"""
    from fluxmi import synth
    from modules.depth import DepthAnythingNative

    cfg = dr.tiny_config(**over)
    sd = synth.make_depth_anything_state_dict(cfg, SEED + 1)
    nat = DepthAnythingNative(cfg)
    nat.load_state_dict(sd, strict=True)
    ps, psd = nat.padded_sizes(), nat.padded_state_dict()
    assert all(n % 128 == 0 for n in ps["neck"] + [ps["fusion"], ps["head1"]]) and ps["head"] % 32 == 0 and ps["head1"] <= 256
    assert set(psd) == set(nat.state_dict())
    for k, v in psd.items():
        o = sd[k]
        assert all(a >= b for a, b in zip(v.shape, o.shape)), k
        block = tuple(slice(0, n) for n in o.shape)
        assert torch.equal(v[block], o), k
        rest = v.clone()
        rest[block] = 0
        assert not rest.any(), f"{k}: a pad is not zero"
    assert psd["neck.convs.0.weight"].shape[:2] == (ps["fusion"], ps["neck"][0]) and psd["head.conv2.weight"].shape[:2] == (ps["head"], ps["head1"])
    for g in ((3, 5), (1, 1)):
        pix = dr.pixel_values(2, *g, seed=3)
        a = dr.forward(sd, cfg, pix, torch.bfloat16)
        b = dr.forward(psd, cfg, pix, torch.bfloat16)
        assert torch.equal(a, b), f"padded vs unpadded under bf16 rounding points at {g}: rel-L2 {dr.rel_l2(b, a):.3e}"
        a64 = dr.forward({k: v.double() for k, v in sd.items()}, cfg, pix)
        b64 = dr.forward({k: v.double() for k, v in psd.items()}, cfg, pix)
        assert dr.rel_l2(b64, a64) <= 1e-13
    # the backbone's pads: heads to 64, fc1 / fc2 to 256, the patch matrix's K to 640
    p = nat.layer_weights(0)
    assert p["wqk"].shape == (2 * 2 * 64, 128) and p["w1"].shape[0] % 256 == 0 and p["w2"].shape[1] % 256 == 0
    assert nat.layer_weights("embed")["w"].shape == (128, 640) and not nat.layer_weights("embed")["w"][:, 588:].any()
    assert torch.equal(p["l1"], sd["backbone.encoder.layer.0.layer_scale1.lambda1"].bfloat16())


# ---- position embedding, input size ----------------------------------------------------------------------------------------------------------
def test_position_embedding_interpolation_is_transformers_bit_for_bit(tiny):
    from modules.depth import interpolate_position_embedding

    cfg, sd, _ = tiny
    hf = dr.hf_model(cfg)
    hf.load_state_dict(sd, strict=True)
    emb = hf.backbone.embeddings
    pos = sd["backbone.embeddings.position_embeddings"]
    for gh, gw in dr.GRIDS + [(37, 37), (37, 36), (20, 50)]:
        with torch.no_grad():
            want = emb.interpolate_pos_encoding(torch.zeros(1, gh * gw + 1, pos.shape[-1]), 14 * gh, 14 * gw)[0]
        got = interpolate_position_embedding(pos, gh, gw)
        assert got.dtype == torch.float32 and torch.equal(got, want), (gh, gw)
        assert torch.equal(dr.interpolate_pos(pos, gh, gw), want), (gh, gw)
    assert torch.equal(interpolate_position_embedding(pos, 37, 37), pos[0])


def test_input_size_rule_and_preprocessing_are_the_dpt_image_processors():
    from PIL import Image
    from transformers.models.dpt.image_processing_pil_dpt import DPTImageProcessorPil

    from modules.depth import IMAGENET_MEAN, IMAGENET_STD, DepthAnythingNative, depth_input_size

    assert [depth_input_size(w, h) for w, h in ((640, 480), (480, 640), (518, 518), (1024, 300))] == [(686, 518), (518, 686), (518, 518), (518, 154)]
    nat = DepthAnythingNative(dr.tiny_config())
    rng = np.random.default_rng(0)
    for res in (518, 140):
        proc = DPTImageProcessorPil(do_resize=True, size={"height": res, "width": res}, keep_aspect_ratio=True, ensure_multiple_of=14, resample=3,
                                    do_rescale=True, do_normalize=True, image_mean=list(IMAGENET_MEAN), image_std=list(IMAGENET_STD), do_pad=False)
        for w, h in ((640, 480), (480, 640), (518, 518), (1024, 300), (97, 203)):
            img = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
            want = proc(images=img, return_tensors="pt").pixel_values
            gw, gh = depth_input_size(w, h, res)
            assert tuple(want.shape) == (1, 3, gh, gw) and gh % 14 == 0 and gw % 14 == 0, (w, h, res)
            assert torch.equal(nat.preprocess(img, res), want), (w, h, res)
    assert depth_input_size(1024, 8, 518) == (518, 14), "a side that rounds to 0 becomes one patch"


# ---- depth -> map ----------------------------------------------------------------------------------------------------------------------------
def test_depth_to_map_reference():
    d = dr.depth_samples(3, 11, 17)
    # the identity size: the source pixels themselves, so the end points of minmax are exactly 0 and 255
    t = dr.depth_to_map_f64(d, 11, 17, "minmax")
    by = dr.map_bytes(t)
    for b in range(3):
        assert by[b].min() == 0 and by[b].max() == 255
        assert by[b].flat[np.argmin(d[b])] == 0 and by[b].flat[np.argmax(d[b])] == 255
    # any size stays inside 0..255 (a bilinear blend cannot leave the source's range)
    for H, W in ((1, 1), (5, 40), (33, 20), (64, 64)):
        t = dr.depth_to_map_f64(d, H, W, "minmax")
        assert t.shape == (3, H, W) and t.min() >= -1e-9 and t.max() <= 255 + 1e-9
    const = np.full((2, 7, 9), 3.25, dtype=np.float32)
    assert not dr.map_bytes(dr.depth_to_map_f64(const, 20, 30, "minmax")).any(), "a constant image gives 0"
    raw = np.array([[[-4.0, 0.4, 0.5], [1.49, 254.6, 300.0]]], dtype=np.float32)
    assert dr.map_bytes(dr.depth_to_map_f64(raw, 2, 3, "raw")).tolist() == [[[0, 0, 1], [1, 255, 255]]]
    # a sample's map depends on that sample alone
    alone = dr.depth_to_map_f64(d[1:2], 20, 30, "minmax")
    assert np.array_equal(alone[0], dr.depth_to_map_f64(d, 20, 30, "minmax")[1])
    # under 1 % of the GPU test's pixels sit within 2^-10 of a rounding step
    for (h, w), (H, W) in dr.MAP_CASES:
        for mode in ("minmax", "raw"):
            assert dr.map_excused(dr.depth_to_map_f64(dr.depth_samples(3, h, w, 1), H, W, mode)).mean() < 0.01, (h, w, H, W, mode)


# ---- ops / pipeline / HTTP refusals ------------------------------------------------------------------------------------------------------------
def test_ops_refuse_by_name():
    from fluxmi import ops

    x = torch.zeros(2, 4, 4, 8, dtype=torch.bfloat16)
    for call in (lambda: ops.unary(x, "relu"), lambda: ops.resize_bilinear(x, (3, 3)), lambda: ops.im2col3x3_s2(x),
                 lambda: ops.depth_to_map(torch.zeros(1, 4, 4), (8, 8))):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    assert ops.conv3x3_s2_hw(1, 1) == (1, 1) and ops.conv3x3_s2_hw(3, 5) == (2, 3) and ops.conv3x3_s2_hw(4, 4) == (2, 2) and ops.conv3x3_s2_hw(37, 37) == (19, 19)


def test_pipeline_refusals():
    from test_preprocess_cpu import make_pipe

    g = torch.Generator().manual_seed(1)
    prompt = {"txt": 0.1 * torch.randn(1, 32, 128, generator=g), "vec": torch.randn(1, 64, generator=g)}
    KW = dict(width=64, height=64, num_steps=4, seed=7, silent=True, output_type="latent")
    photo = np.random.default_rng(0).integers(0, 256, (48, 40, 3), dtype=np.uint8)
    pipe = make_pipe(extra=64)
    # without a depth model the kind is refused, naming the config field; "depth" stays refused and now points at the kind
    with pytest.raises(ValueError, match="depth_path"):
        pipe.generate(prompt, control_image=photo, control_preprocess="depth_anything", **KW)
    with pytest.raises(ValueError, match="depth_path"):
        pipe.preprocess_control(photo, "depth_anything", 64, 64)
    with pytest.raises(ValueError, match="control_preprocess='depth'.*depth_anything"):
        pipe.generate(prompt, control_image=photo, control_preprocess="depth", **KW)
    with pytest.raises(ValueError, match="control_preprocess needs control_image"):
        pipe.generate(prompt, control_preprocess="depth_anything", **KW)
    pipe.depth_model = object()  # present: the argument checks speak next, still before any work
    for bad in (13, 1037, 0, -518, 518.0, True, "518"):
        with pytest.raises(ValueError, match="depth_resolution=.*14..1036"):
            pipe.generate(prompt, control_image=photo, control_preprocess="depth_anything", depth_resolution=bad, **KW)
    with pytest.raises(ValueError, match="depth_normalize='bicubic'"):
        pipe.generate(prompt, control_image=photo, control_preprocess="depth_anything", depth_normalize="bicubic", **KW)
    with pytest.raises(ValueError, match="patch grid.*5477 tokens"):
        pipe.generate(prompt, control_image=photo, control_preprocess="depth_anything", depth_resolution=1036,
                      **{**KW, "width": 2048, "height": 1024})
    for extra in (dict(depth_resolution=300), dict(depth_normalize="raw")):
        with pytest.raises(ValueError, match="belong to control_preprocess"):
            pipe.generate(prompt, control_image=photo, **extra, **KW)
        with pytest.raises(ValueError, match="belong to control_preprocess"):
            pipe.generate(prompt, control_image=photo, control_preprocess="canny", **extra, **KW)
    with pytest.raises(ValueError, match="img_cond / controlnet_cond"):
        pipe.generate(prompt, control_preprocess="depth_anything", img_cond=torch.zeros(1, 16, 64), **KW)
    assert pipe.model.calls == []
    # the other kinds' calls carry no depth argument: what preprocess_control received before, it receives now
    seen = []
    pipe.preprocess_control = lambda *a, **k: seen.append(k) or torch.zeros(64, 64, 3, dtype=torch.uint8)
    pipe.prepare_control_conditioning = lambda *a, **k: torch.zeros(1, 16, 64)
    pipe.generate(prompt, control_image=photo, control_preprocess="canny", **KW)
    pipe.generate(prompt, control_image=photo, control_preprocess="depth_anything", depth_resolution=140, **KW)
    assert set(seen[0]) == {"canny_low", "canny_high", "canny_l2", "blur_sigma"}
    assert seen[1]["depth_resolution"] == 140 and seen[1]["depth_normalize"] == "minmax"


def test_http_fields():
    from fastapi.testclient import TestClient

    import api

    calls = []

    class Stub:
        def generate(self, **kw):
            calls.append(kw)
            return io.BytesIO(b"\xff\xd8jpeg-bytes\xff\xd9")

    f = api.GenerateArgs.model_fields
    for k in ("depth_resolution", "depth_normalize"):
        assert k in f and f[k].default is None
    api.app.state.model = Stub()
    c = TestClient(api.app)
    base = {"prompt": "a cat on a bench", "width": 512, "height": 512, "num_steps": 4, "seed": 7}
    assert c.post("/generate", json=base).status_code == 200
    assert set(calls[-1]) == {"prompt", "width", "height", "num_steps", "guidance", "seed", "strength", "init_image"}
    r = c.post("/generate", json={**base, "control_image": "photo.png", "control_preprocess": "depth_anything"})
    assert r.status_code == 200 and r.content.startswith(b"\xff\xd8")
    assert calls[-1]["control_preprocess"] == "depth_anything" and "depth_resolution" not in calls[-1] and "depth_normalize" not in calls[-1]
    r = c.post("/generate", json={**base, "controlnet_image": "photo.png", "control_preprocess": "depth_anything", "depth_resolution": 392,
                                  "depth_normalize": "raw"})
    assert r.status_code == 200 and (calls[-1]["depth_resolution"], calls[-1]["depth_normalize"]) == (392, "raw")
    for bad in ({"control_preprocess": "depth"}, {"depth_resolution": 13}, {"depth_resolution": 1037}, {"depth_resolution": 518.5},
                {"depth_normalize": "max"}):
        assert c.post("/generate", json={**base, **bad}).status_code == 422, bad
