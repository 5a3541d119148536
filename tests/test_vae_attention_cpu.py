"""The streaming VAE attention without a GPU: the error gate of tests/vae_attention_ref.py has the power to see each defect the kernel could
have (the model with one mutation must fail it), the C entry's refusals (they come before any launch), and the configuration surface
(ModelSpec.vae_attention -> AutoEncoder.attention -> FluxPipeline._check_tiles)."""
import numpy as np
import pytest
import torch

import vae_attention_ref as var
from helper_refs import rbf64
from test_flowedit_cpu import make_pipe

PS = [63, 65, 200, 1089]
DS = [64, 512]


# ---- the gate ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("P", [1] + PS)
def test_reference_and_model_sit_inside_the_gate(P, D):
    """the fp64 reference rounded once to bf16, and the model itself, pass on every family: the gate asks nothing the arithmetic cannot give"""
    for fam in var.FAMILIES:
        q, k, v, b = var.inputs(fam, 1, P, D, seed=1)
        g = var.gate(q, k, v, b)
        var.assert_close(rbf64(g["ref"]), g, f"rounded fp64 {fam} P={P} D={D}")
        var.assert_close(var.model(q, k, v, b), g, f"model {fam} P={P} D={D}")
        assert g["r_model"] <= 1.0, f"{fam} P={P} D={D}: the model itself is outside u (|ref| + A): {g['r_model']:.3f}"


@pytest.mark.parametrize("mut", var.MUTANTS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("P", PS)
def test_gate_rejects_mutant(P, D, mut):
    """every defect is seen on the probe_last family at every size.  One exception that is none: at P <= KEY_TILE there is ONE key tile, the
    rescale factor only ever multiplies the zero start values, and the model without it IS the model -- asserted bit for bit instead."""
    q, k, v, b = var.inputs("probe_last", 3, P, D, seed=2)
    g = var.gate(q, k, v, b)
    got = var.model(q, k, v, b, mut=mut)
    if mut == "no_rescale" and P <= var.KEY_TILE:
        assert torch.equal(got.view(torch.int16), var.model(q, k, v, b).view(torch.int16))
        return
    with pytest.raises(AssertionError, match="elements beyond|rel-L2"):
        var.assert_close(got, g, f"mutant {mut} P={P} D={D}")


# ---- the C entry ------------------------------------------------------------------------------------------------------------------------
def test_lib_entry_and_abi():
    from fluxmi import _lib

    assert "fluxmi_vae_attention" in _lib.EXPORTS and hasattr(_lib.lib, "fluxmi_vae_attention")
    assert len(_lib._SIGS["fluxmi_vae_attention"][0]) == 16
    assert _lib.lib.fluxmi_abi_version() == 5 and _lib.ABI_VERSION == 5


@pytest.mark.parametrize("kw, match", [
    (dict(D=128), "D=128"),
    (dict(D=0), "D=0"),
    (dict(P=0), "P=0"),
    (dict(Pp=100), "Pp=100"),
    (dict(P=129), "Pp=128"),
    (dict(ld_qk=516), "q / k strides"),
    (dict(bs_qk=4), "q / k strides"),
    (dict(ld_vt=132), "V\\^T strides"),
    (dict(ld_vt=64), "V\\^T strides"),
    (dict(ld_out=515), "out strides"),
    (dict(q=0x1008), "16-byte"),
    (dict(k=0x2004), "16-byte"),
    (dict(vt=0x3002), "16-byte"),
    (dict(out=0x4008), "16-byte"),
    (dict(v_bias=0x5008), "16-byte"),
    (dict(B=0), "B=0"),
])
def test_entry_refuses_before_any_launch(kw, match):
    """the refusals are host-side checks ahead of the launch: the pointers below are never dereferenced (and there is no GPU here)"""
    import ctypes as C

    from fluxmi import _lib

    a = dict(q=0x1000, k=0x2000, ld_qk=512, bs_qk=512 * 128, vt=0x3000, ld_vt=128, bs_vt=128 * 512, out=0x4000, ld_out=512, bs_out=512 * 100,
             v_bias=0x5000, D=512, P=100, Pp=128, B=2)
    a.update(kw)
    vp = lambda x: C.c_void_p(x)
    rc = _lib.lib.fluxmi_vae_attention(vp(a["q"]), vp(a["k"]), a["ld_qk"], a["bs_qk"], vp(a["vt"]), a["ld_vt"], a["bs_vt"], vp(a["out"]), a["ld_out"],
                                       a["bs_out"], vp(a["v_bias"]), a["D"], a["P"], a["Pp"], a["B"], None)
    assert rc == 1
    import re

    msg = _lib.lib.fluxmi_last_error().decode()
    assert re.search(match, msg), msg


# ---- configuration ----------------------------------------------------------------------------------------------------------------------
def test_model_spec_and_autoencoder_carry_the_mode():
    from modules.autoencoder import ATTENTION_MODES, AutoEncoder, AutoEncoderParams
    from util import ModelSpec

    assert ATTENTION_MODES == ("gemm", "streaming")
    assert ModelSpec.model_fields["vae_attention"].default == "gemm"
    ae = AutoEncoder(AutoEncoderParams(resolution=32, in_channels=3, ch=32, out_ch=3, ch_mult=[1, 2], num_res_blocks=1, z_channels=4,
                                       scale_factor=0.3611, shift_factor=0.1159))
    assert ae.attention == "gemm"
    ae.attention = "streaming"
    assert ae.attention == "streaming"
    with pytest.raises(ValueError, match="vae_attention"):
        ae.attention = "flash"
    assert ae.attention == "streaming"


def test_load_autoencoder_and_pipeline_constructor_carry_the_mode():
    import types

    import util
    from flux_pipeline import FluxPipeline
    from modules.autoencoder import AutoEncoder, AutoEncoderParams

    params = AutoEncoderParams(resolution=32, in_channels=3, ch=32, out_ch=3, ch_mult=[1, 2], num_res_blocks=1, z_channels=4,
                               scale_factor=0.3611, shift_factor=0.1159)
    sd = AutoEncoder(params).state_dict()
    for mode in ("gemm", "streaming"):
        cfg = types.SimpleNamespace(ae_params=params, ae_device="cpu", vae_attention=mode)
        assert util.load_autoencoder(cfg, sd).attention == mode
    with pytest.raises(ValueError, match="vae_attention"):
        util.load_autoencoder(types.SimpleNamespace(ae_params=params, ae_device="cpu", vae_attention="tiled"), sd)

    class Model:
        def to(self, device):
            return self

    base = dict(offload_text_encoder=False, offload_vae=False, offload_flow=False, compile_blocks=False, compile_extras=False)
    ae = AutoEncoder(params)
    pipe = FluxPipeline("flux-dev", model=Model(), ae=ae, flux_device="cpu", ae_device="cpu", clip_device="cpu", t5_device="cpu",
                        config=types.SimpleNamespace(vae_attention="streaming", **base))
    assert pipe.vae_attention == "streaming" and ae.attention == "streaming"
    pipe = FluxPipeline("flux-dev", model=Model(), ae=ae, flux_device="cpu", ae_device="cpu", clip_device="cpu", t5_device="cpu",
                        config=types.SimpleNamespace(**base))
    assert pipe.vae_attention == "gemm" and ae.attention == "gemm"
    with pytest.raises(ValueError, match="vae_attention"):
        FluxPipeline("flux-dev", model=Model(), ae=ae, flux_device="cpu", ae_device="cpu", clip_device="cpu", t5_device="cpu",
                     config=types.SimpleNamespace(vae_attention="none", **base))


PHOTO = np.zeros((64, 64, 3), dtype=np.uint8)
BIG = dict(width=2048, height=2048, tile_size=1024, tile_overlap=0, num_steps=8, seed=1, silent=True)


def check_args(**kw):
    """what generate hands _check_tiles (test_windows_cpu.test_check_tiles_plans), for a tiled request"""
    a = dict(sampler="euler", eta=1.0, s_noise=1.0, noise_seed=None, guidance_mode="cfg", guidance_rescale=0.0, zero_init_steps=0, apg_eta=1.0,
             apg_norm_threshold=0.0, apg_momentum=0.0, inpaint_mask=None, reference_image=None, redux_image=None, regions=None,
             source_prompt=None, mask_image=None, control_image=None, img_cond=None, inpaint_differential=False, controlnet_image=None,
             controlnet_cond=None, ip_adapter_image=None, ip_adapter_image_embeds=None, negative_ip_adapter_image=None, cache_threshold=0.0,
             preview_every=0, preview_factors=None, on_step=None, sigma_schedule=None, negative_prompt=None, true_cfg_scale=1.0,
             true_cfg_interval=(0.0, 1.0), num_images=1, prompt="a wide valley", output_type="jpeg", init_image=None, tile_weight="cosine")
    a.update(kw)
    return a


def test_default_pipeline_refuses_2048_as_before():
    from flux_pipeline import FluxPipeline

    assert FluxPipeline.vae_attention == "gemm" and FluxPipeline.VAE_MAX_LATENT_PIXELS == 46340
    with pytest.raises(ValueError, match="tile_size.*VAE"):
        make_pipe().generate("a wide valley", **{**BIG, "output_type": "jpeg"})
    with pytest.raises(ValueError, match="tile_size.*VAE"):
        make_pipe().generate("a wide valley", **{**BIG, "init_image": PHOTO, "strength": 0.5, "output_type": "latent"})


def test_streaming_pipeline_admits_2048_and_refuses_above_its_bound():
    """_check_tiles against the untouchable stubs (any attribute access on pipe.ae raises): it reads pipe.vae_attention only"""
    from flux_pipeline import FluxPipeline

    pipe = make_pipe()
    pipe.vae_attention = "streaming"
    bound = FluxPipeline.VAE_MAX_LATENT_PIXELS_STREAMING
    assert 65536 <= bound < 131072  # 64 P x 256 channels x 2 bytes < 4 GiB
    big = dict(width=2048, height=2048, tile_size=1024, tile_overlap=0)
    plan = pipe._check_tiles(check_args(**big))
    assert (plan.ny, plan.nx) == (2, 2)
    plan = pipe._check_tiles(check_args(**big, init_image=PHOTO, output_type="latent"))
    assert (plan.ny, plan.nx) == (2, 2)
    # 4096 x 2048 = 131072 latent pixels: one past the bound
    over = dict(width=4096, height=2048, tile_size=1024, tile_overlap=0)
    assert (4096 // 8) * (2048 // 8) == bound + 1
    with pytest.raises(ValueError, match="tile_size.*VAE.*streaming"):
        pipe._check_tiles(check_args(**over))
    with pytest.raises(ValueError, match="tile_size.*init_image.*VAE"):
        pipe._check_tiles(check_args(**over, init_image=PHOTO, output_type="latent"))
    assert pipe._check_tiles(check_args(**over, output_type="latent")) is not None  # nothing decodes, nothing encodes
    # 2816 x 2816 = 123904 latent pixels: inside
    assert pipe._check_tiles(check_args(width=2816, height=2816, tile_size=1408, tile_overlap=0)) is not None


def test_bad_mode_is_refused():
    pipe = make_pipe()
    pipe.vae_attention = "tiled"
    with pytest.raises(ValueError, match="vae_attention"):
        pipe._check_tiles(check_args(width=2048, height=2048, tile_size=1024, tile_overlap=0))


def test_streaming_refuses_other_mid_widths_by_name():
    from modules.autoencoder import AutoEncoder, AutoEncoderParams

    ae = AutoEncoder(AutoEncoderParams(resolution=32, in_channels=3, ch=32, out_ch=3, ch_mult=[1, 4], num_res_blocks=1, z_channels=4,
                                       scale_factor=0.3611, shift_factor=0.1159))
    ae.attention = "streaming"
    with pytest.raises(ValueError, match="streaming.*64 or 512.*128"):
        ae._attn_streaming(torch.zeros(1, 4, 4, 128, dtype=torch.bfloat16), ae.decoder.mid.attn_1)


def test_large_batches_run_image_by_image():
    """num_images multiplies the rows of every convolution: a batch whose rows would pass the 32-bit descriptor is split, one below is not"""
    from modules.autoencoder import AutoEncoder, AutoEncoderParams

    ae = AutoEncoder(AutoEncoderParams(resolution=32, in_channels=3, ch=32, out_ch=3, ch_mult=[1, 2], num_res_blocks=1, z_channels=4,
                                       scale_factor=0.3611, shift_factor=0.1159))
    seen = []
    fn = lambda t: (seen.append(tuple(t.shape)), t + 1)[1]
    t = torch.zeros(2, 4, 3, 5)
    assert ae._per_image(fn, t, 65536) is not None and seen == [(1, 4, 3, 5), (1, 4, 3, 5)]
    assert ae._per_image(fn, t, 65535) is None and ae._per_image(fn, t[:1], 131072) is None and len(seen) == 2
