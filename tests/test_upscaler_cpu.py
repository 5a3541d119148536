"""The ESRGAN upscaler without a GPU: the per-element gate of tests/upscaler_ref.py accepts the fp32 model in two summation orders and
rejects every mutant on every input family; both checkpoint key layouts map onto one network; geometry inference; the refusals; synthetic
state dicts through .safetensors; the new /generate fields."""
import pytest
import torch

import upscaler_ref as ur

ACCEPT_ARMS = [dict(ur.ARMS_NONE), dict(ur.ARMS_NONE, bias=True, act=True), dict(ur.ARMS_NONE, bias=True, act=True, r1=True, r2=True)]


@pytest.mark.parametrize("cin", [16, 64, 96, 128, 160, 192])
def test_gate_accepts_the_model_in_two_orders(cin):
    worst = 0.0
    for fam in ur.FAMILIES:
        inp = ur.conv_inputs(fam, 2, 9, 11, cin, 32, seed=1)
        for arms in ACCEPT_ARMS:
            g = ur.conv_gate(inp, arms)
            for order in (0, 1):
                n_bad, r = ur.conv_check(ur.conv_model(inp["xbuf"], order=order, **ur.conv_args(inp, arms)), g)
                worst = max(worst, r)
                assert n_bad == 0, f"{fam} Cin={cin} order {order}: the gate rejects the model ({n_bad} elements, worst {r:.3f})"
    print(f"CONV_DENSE_MODEL Cin={cin}: worst err/bound of the fp32 model {worst:.3f} (un-margined bound = 1)")
    assert worst <= 1.0, "the fp32 model should stay inside the un-margined bound"


@pytest.mark.parametrize("cin", [16, 96])
@pytest.mark.parametrize("mut", ur.MUTANTS)
def test_gate_rejects_every_mutant_on_every_family(mut, cin):
    arms = ur.MUTANT_ARMS[mut]
    up = arms["upsample"]
    for fam in ur.FAMILIES:
        inp = ur.conv_inputs(fam, 2, 10 // up, 12 // up, cin, 32, seed=2, upsample=up)
        g = ur.conv_gate(inp, arms)
        assert ur.conv_check(ur.conv_model(inp["xbuf"], **ur.conv_args(inp, arms)), g)[0] == 0
        n_bad, r = ur.conv_check(ur.conv_model(inp["xbuf"], mut=mut, **ur.conv_args(inp, arms)), g)
        assert n_bad > 0, f"mutant {mut} passes the gate on {fam} at Cin={cin} (worst err/bound {r:.3f})"


def test_reference_upsample_is_nearest():
    x = torch.arange(2 * 3 * 1, dtype=torch.float32).reshape(1, 2, 3, 1)
    up = ur._gather(x, 2)
    want = torch.nn.functional.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(up, want)


def test_reference_convolution_is_conv2d():
    inp = ur.conv_inputs("randn", 2, 5, 7, 32, 8, seed=3)
    x = inp["xbuf"][..., :32]
    ref, _ = ur.conv_ref64(x, inp["w"], inp["bias"])
    want = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), inp["w"].double().permute(0, 3, 1, 2), inp["bias"].double(), padding=1)
    assert torch.allclose(ref, want.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)


# ---- checkpoints -------------------------------------------------------------------------------------------------------------------
def test_both_key_layouts_map_onto_the_same_network():
    from fluxmi import synth
    from modules import upscaler as up

    new = synth.make_rrdbnet_state_dict(2, 64, 32, 4, seed=5, layout="new")
    old = synth.make_rrdbnet_state_dict(2, 64, 32, 4, seed=5, layout="old")
    assert "model.1.sub.1.RDB3.conv5.0.weight" in old and "model.1.sub.2.weight" in old and "model.10.bias" in old
    n_new, l_new = up.normalize_state_dict({"params_ema": new})
    n_old, l_old = up.normalize_state_dict(old)
    assert (l_new, l_old) == ("new", "old") and set(n_new) == set(n_old)
    assert all(torch.equal(n_new[k], n_old[k]) for k in n_new)
    a, b = up.RRDBNet(new, device="cpu"), up.RRDBNet({"params": old}, device="cpu")
    assert all(torch.equal(a.layers[k][0], b.layers[k][0]) and torch.equal(a.layers[k][1], b.layers[k][1]) for k in a.layers)
    w2, b2, cout = a.layers["conv_last"]
    assert tuple(w2.shape) == (32, 3, 3, 64) and cout == 3 and not w2[3:].any() and not b2[3:].any()
    assert tuple(a.layers["conv_first"][0].shape) == (64, 3, 3, 16) and not a.layers["conv_first"][0][..., 3:].any()


@pytest.mark.parametrize("scale,in_ch", [(4, 3), (2, 12), (1, 48)])
def test_geometry_is_inferred_from_the_state_dict(scale, in_ch):
    from fluxmi import synth
    from modules import upscaler as up

    net = up.RRDBNet(synth.make_rrdbnet_state_dict(3, 48, 16, scale, seed=1), device="cpu")
    assert (net.num_block, net.nf, net.gc, net.in_ch, net.scale) == (3, 48, 16, in_ch, scale)
    assert net.layers["conv_first"][0].shape[-1] == -(-in_ch // 16) * 16
    assert net.memory_estimate(1, 1024, 1024) > 0


def test_foreign_checkpoints_are_refused_by_name():
    from fluxmi import synth
    from modules import upscaler as up

    z = torch.zeros(1)
    with pytest.raises(up.UpscalerFormatError, match="SRVGGNetCompact"):
        up.normalize_state_dict({"body.0.weight": z, "body.1.weight": z, "body.2.weight": z})
    with pytest.raises(up.UpscalerFormatError, match="SwinIR"):
        up.normalize_state_dict({"conv_first.weight": z, "layers.0.residual_group.blocks.0.attn.qkv.weight": z})
    with pytest.raises(up.UpscalerFormatError, match="DAT"):
        up.normalize_state_dict({"conv_first.weight": z, "before_RG.0.weight": z, "layers.0.blocks.0.attn.attns.0.attn.temperature": z})
    old = synth.make_rrdbnet_state_dict(1, 64, 32, 4, layout="old")
    x2 = {("model.13" + k[len("model.10"):] if k.startswith("model.10") else k): v for k, v in old.items()}
    with pytest.raises(up.UpscalerFormatError, match="other than 4"):
        up.normalize_state_dict(x2)
    new = synth.make_rrdbnet_state_dict(1, 64, 32, 4)
    with pytest.raises(up.UpscalerFormatError, match="unexpected key"):
        up.RRDBNet(dict(new, **{"extra.weight": z}), device="cpu")
    with pytest.raises(up.UpscalerFormatError, match="no conv_hr"):
        up.RRDBNet({k: v for k, v in new.items() if not k.startswith("conv_hr")}, device="cpu")
    with pytest.raises(up.UpscalerFormatError, match="gc=24"):
        up.RRDBNet(synth.make_rrdbnet_state_dict(1, 64, 24, 4), device="cpu")
    bad = dict(new)
    bad["conv_first.weight"] = torch.zeros(64, 5, 3, 3)
    with pytest.raises(up.UpscalerFormatError, match="5 channels"):
        up.RRDBNet(bad, device="cpu")


def test_synthetic_state_dicts_round_trip_through_safetensors(tmp_path):
    from safetensors.torch import save_file

    import util
    from fluxmi import synth

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    assert util.ModelSpec.model_fields["upscaler_path"].default is None and util.load_upscaler(cfg, device="cpu") is None
    cfg.upscaler_path = str(tmp_path / "missing.safetensors")
    assert util.load_upscaler(cfg, device="cpu") is None  # nothing is downloaded, nothing is guessed
    for layout in ("new", "old"):
        sd = synth.make_rrdbnet_state_dict(2, 64, 32, 4, seed=9, layout=layout)
        path = tmp_path / f"rrdb_{layout}.safetensors"
        save_file(sd, str(path))
        cfg.upscaler_path = str(path)
        net = util.load_upscaler(cfg, device="cpu")
        assert (net.layout, net.num_block, net.nf, net.gc, net.scale) == (layout, 2, 64, 32, 4)
    pth = tmp_path / "rrdb.pth"
    torch.save({"params_ema": synth.make_rrdbnet_state_dict(1, 64, 32, 2, seed=9)}, str(pth))
    cfg.upscaler_path = str(pth)
    assert util.load_upscaler(cfg, device="cpu").scale == 2


# ---- requests ----------------------------------------------------------------------------------------------------------------------
def test_pipeline_refusals_fire_up_front():
    from flux_pipeline import FluxPipeline
    from fluxmi import synth
    from modules.upscaler import RRDBNet

    p = object.__new__(FluxPipeline)
    p.upscaler, p.ae = None, object()
    for kw in (dict(upscale=True), dict(init_upscale=True, init_image=torch.zeros(8, 8, 3, dtype=torch.uint8))):
        with pytest.raises(ValueError, match="upscaler_path"):
            p.generate("a prompt", **kw)
    with pytest.raises(ValueError, match="upscaler_path"):
        p.upscale(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    p.upscaler = RRDBNet(synth.make_rrdbnet_state_dict(1, 64, 32, 4), device="cpu")
    with pytest.raises(ValueError, match="latent"):
        p.generate("a prompt", upscale=True, output_type="latent")
    with pytest.raises(ValueError, match="needs init_image"):
        p.generate("a prompt", init_upscale=True)
    with pytest.raises(ValueError, match="launch grid"):
        p.generate("a prompt", upscale=True, output_type="uint8", num_images=65536, width=64, height=64)
    with pytest.raises(ValueError, match="launch grid"):
        p.upscaler.check_input(1, 16 * 65536 // 4, 8)
    x2 = RRDBNet(synth.make_rrdbnet_state_dict(1, 64, 32, 2), device="cpu")
    with pytest.raises(ValueError, match="multiples of 2"):
        x2.check_input(1, 9, 8)
    with pytest.raises(ValueError, match="uint8"):
        p.upscale(torch.zeros(1, 8, 8, 3))


def test_http_upscale_fields():
    import io

    from fastapi.testclient import TestClient

    import api

    f = api.GenerateArgs.model_fields
    assert f["upscale"].default is False and f["init_upscale"].default is False
    a = api.GenerateArgs(prompt="p", upscale=True, init_upscale=True)
    assert a.upscale is True and a.init_upscale is True
    assert {"upscale", "init_upscale"} <= set(api.GenerateArgs.model_json_schema()["properties"])
    calls = []

    class Stub:
        def generate(self, **kw):
            calls.append(kw)
            return io.BytesIO(b"\xff\xd8jpeg\xff\xd9")

    api.app.state.model = Stub()
    c = TestClient(api.app)
    assert c.post("/generate", json={"prompt": "x"}).status_code == 200
    assert "upscale" not in calls[-1] and "init_upscale" not in calls[-1]  # a request that does not ask is the request it was
    assert c.post("/generate", json={"prompt": "x", "upscale": True, "init_image": "in.png", "init_upscale": True}).status_code == 200
    assert calls[-1]["upscale"] is True and calls[-1]["init_upscale"] is True and calls[-1]["init_image"] == "in.png"
    assert c.post("/generate", json={"prompt": "x", "upscale": "maybe"}).status_code == 422
