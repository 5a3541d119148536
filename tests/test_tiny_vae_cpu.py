"""The tiny autoencoder off the GPU: the loader's key styles and refusals, the configuration and HTTP defaults, the refused requests."""
import inspect

import pytest
import torch


def test_loader_key_styles_and_wrong_geometry(tmp_path):
    from safetensors.torch import save_file

    import util
    from fluxmi import synth
    from modules import tiny_vae as tv

    bare = synth.make_taef1_state_dict(seed=3)
    assert "1.weight" in bare and "3.conv.0.weight" in bare and "19.bias" in bare and "7.bias" not in bare
    for prefix in ("decoder.", "decoder.layers."):
        other = synth.make_taef1_state_dict(seed=3, prefix=prefix)
        assert (prefix + ("0.weight" if prefix.endswith("layers.") else "1.weight")) in other
        other["encoder.1.weight"] = torch.zeros(64, 3, 3, 3)  # a full file: the encoder is ignored
        got = tv.normalize_state_dict(other)
        assert set(got) == set(bare) and all(torch.equal(got[k], bare[k]) for k in bare)
    for name, t in (("1.weight", torch.zeros(64, 4, 3, 3)), ("9.conv.2.weight", torch.zeros(32, 64, 3, 3)), ("7.bias", torch.zeros(64)),
                    ("model.0.weight", torch.zeros(1))):
        with pytest.raises(tv.TinyAEFormatError):
            tv.normalize_state_dict(dict(bare, **{name: t}))
    with pytest.raises(tv.TinyAEFormatError, match="19.bias"):
        tv.normalize_state_dict({k: v for k, v in bare.items() if k != "19.bias"})
    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    assert util.ModelSpec.model_fields["tiny_ae_path"].default is None and util.load_tiny_ae(cfg, device="cpu") is None
    cfg.tiny_ae_path = str(tmp_path / "missing.safetensors")
    assert util.load_tiny_ae(cfg, device="cpu") is None  # nothing is downloaded, nothing is guessed
    save_file(bare, str(tmp_path / "taef1.safetensors"))
    torch.save(synth.make_taef1_state_dict(seed=3, prefix="decoder.layers."), str(tmp_path / "taef1.pth"))
    for name in ("taef1.safetensors", "taef1.pth"):
        cfg.tiny_ae_path = str(tmp_path / name)
        net = util.load_tiny_ae(cfg, device="cpu")
        assert (net.scale_factor, net.shift_factor) == (cfg.ae_params.scale_factor, cfg.ae_params.shift_factor)
        assert torch.equal(net.stem[0], bare["1.weight"].permute(0, 2, 3, 1).bfloat16())


def test_defaults_and_refused_requests():
    import api
    from flux_pipeline import FluxPipeline

    assert inspect.signature(FluxPipeline.generate).parameters["decoder"].default == "vae"
    assert api.GenerateArgs.model_fields["decoder"].default is None and api.GenerateArgs(prompt="p", decoder="tiny").decoder == "tiny"
    with pytest.raises(ValueError):
        api.GenerateArgs(prompt="p", decoder="taesd")
    p = object.__new__(FluxPipeline)
    p.tiny_ae, p.ae = None, object()
    with pytest.raises(ValueError, match="tiny_ae_path"):
        p.generate("a prompt", decoder="tiny")
    with pytest.raises(ValueError, match="tiny_ae_path"):
        p.tiny_decode(torch.zeros(1, 16, 2, 2))
    with pytest.raises(ValueError, match="expected one of"):
        p.generate("a prompt", decoder="taesd")
    # previews through the tiny decoder: the default is the latent projection; "tiny" needs the file and preview_every > 0, and is then
    # refused wherever preview_every > 0 is (no on_step, a tiled request, a FlowEdit request)
    assert inspect.signature(FluxPipeline.generate).parameters["preview_decoder"].default == "latent"
    assert api.GenerateArgs.model_fields["preview_decoder"].default is None
    assert api.GenerateArgs(prompt="p", preview_decoder="tiny").preview_decoder == "tiny"
    with pytest.raises(ValueError):
        api.GenerateArgs(prompt="p", preview_decoder="vae")
    pv = dict(on_step=lambda info: True, preview_every=2, preview_decoder="tiny")
    with pytest.raises(ValueError, match="expected one of"):
        p.generate("a prompt", **dict(pv, preview_decoder="vae"))
    with pytest.raises(ValueError, match="tiny_ae_path"):
        p.generate("a prompt", **pv)
    from fluxmi import synth
    from modules.tiny_vae import TinyDecoder

    p.tiny_ae = TinyDecoder(synth.make_taef1_state_dict(), device="cpu")
    with pytest.raises(ValueError, match="preview_every > 0"):
        p.generate("a prompt", **dict(pv, preview_every=0))
    with pytest.raises(ValueError, match="needs on_step"):
        p.generate("a prompt", **dict(pv, on_step=None))
    with pytest.raises(ValueError, match="preview_every > 0"):
        p.generate("a prompt", width=96, height=96, tile_size=64, **pv)
    with pytest.raises(ValueError, match="preview_every > 0"):
        p.generate("a prompt", source_prompt="a source", init_image=torch.zeros(64, 64, 3, dtype=torch.uint8), **pv)
