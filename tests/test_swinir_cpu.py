"""SwinIR without a GPU: geometry inference and dispatch of modules/swinir.py, the refusals by name, and the closed form of
include/fluxmi.h (bias index, region ids, -100) against the reference written from SwinIR's own construction (tests/swinir_ref.py)."""
import pytest
import torch

import swinir_ref as sr

TINY = {"a": dict(embed_dim=60, depths=(2, 2), heads=(2, 2), resi="1conv", scale=4),
        "b": dict(embed_dim=64, depths=(2,), heads=(2,), resi="3conv", scale=2)}


@pytest.mark.parametrize("wrap", [None, "params_ema", "params"])
@pytest.mark.parametrize("cfg", list(TINY))
def test_geometry_round_trips(cfg, wrap):
    from fluxmi import synth
    from modules import swinir

    c = TINY[cfg]
    sd = synth.make_swinir_state_dict(seed=1, wrap=wrap, **c)
    assert swinir.is_swin_family(sd)
    g = swinir.infer_geometry(swinir.unwrap(sd))
    assert (g["embed_dim"], tuple(g["depths"]), tuple(g["heads"]), g["resi"], g["after_body"], g["scale"], g["mlp_hidden"], g["num_feat"]) == \
        (c["embed_dim"], c["depths"], c["heads"], c["resi"], c["resi"], c["scale"], 2 * c["embed_dim"], 64)


def test_read_upscaler_dispatches_by_keys(tmp_path):
    from fluxmi import synth
    from modules import swinir, upscaler

    torch.save(synth.make_swinir_state_dict(seed=2, wrap="params_ema", **TINY["a"]), tmp_path / "swin.pth")
    torch.save(synth.make_rrdbnet_state_dict(1, 64, 32, 4, seed=2), tmp_path / "rrdb.pth")
    net = upscaler.read_upscaler(str(tmp_path / "swin.pth"), device="cpu")
    assert isinstance(net, swinir.SwinIR) and net.scale == 4 and (net.C, net.Cp) == (60, 64)
    assert isinstance(upscaler.read_upscaler(str(tmp_path / "rrdb.pth"), device="cpu"), upscaler.RRDBNet)


P0, Z = "layers.0.residual_group.blocks.0.", torch.zeros(1)
VARIANTS = {  # the word the refusal must hold -> (keys added to a good checkpoint, key prefixes dropped from it)
    "pixelshuffle": ({"upsample.0.weight": Z}, ()), "pixelshuffledirect": ({"upsample.0.weight": Z}, ("conv_before_upsample",)),
    "denoise": ({}, ("conv_before_upsample", "conv_up", "conv_hr")),
    "window 7": ({P0 + "attn.relative_position_bias_table": torch.zeros(169, 2)}, ()),
    "window 16": ({P0 + "attn.relative_position_bias_table": torch.zeros(961, 2)}, ()),
    "ape": ({"absolute_pos_embed": Z}, ()), "Swin2SR": ({P0 + "attn.logit_scale": Z}, ()), "HAT": ({P0 + "conv_block.cab.0.weight": Z}, ()),
    "unexpected key": ({"conv_extra.weight": Z}, ()), "expected": ({P0 + "attn.proj.weight": torch.zeros(60, 30)}, ()),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_refused_by_name(name):
    from fluxmi import synth
    from modules import swinir
    from modules.upscaler import UpscalerFormatError

    add, drop = VARIANTS[name]
    sd = {k: v for k, v in synth.make_swinir_state_dict(seed=3, **TINY["a"]).items() if not k.startswith(drop or ("\0",))}
    with pytest.raises(UpscalerFormatError, match=name):
        swinir.SwinIR({**sd, **add}, device="cpu")


@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("H,W", [(8, 8), (8, 16), (16, 8), (24, 16)])
def test_closed_form_equals_swinir_construction(H, W, shift):
    """per window: softmax(q k^T scale + table[(ya - yb + 7) * 15 + xa - xb + 7] + mask) v with the header's rolled coordinates and region ids"""
    g = torch.Generator().manual_seed(H * 100 + W + shift)
    B, nh, hd, scale = 2, 3, 5, 0.4
    q, k, v = (torch.randn(B, H, W, nh, hd, generator=g, dtype=torch.float64) for _ in range(3))
    table = torch.randn(225, nh, generator=g, dtype=torch.float64)
    ref, _ = sr.window_attention_ref64(q, k, v, table, shift, scale)
    ty, tx = torch.arange(64) // 8, torch.arange(64) % 8
    idx = (ty[:, None] - ty[None, :] + 7) * 15 + (tx[:, None] - tx[None, :] + 7)
    region = lambda i, n: (i >= n - 8).long() + (i >= n - 4).long()  # noqa: E731
    out = torch.empty_like(ref)
    for wy in range(H // 8):
        for wx in range(W // 8):
            i, j = 8 * wy + ty, 8 * wx + tx                  # rolled pixels of the window's tokens
            sy, sx = (i + shift) % H, (j + shift) % W        # their source pixels
            rid = 3 * region(i, H) + region(j, W)
            mask = torch.where(rid[:, None] != rid[None, :], -100.0, 0.0) if shift else torch.zeros(64, 64)
            qw, kw, vw = (t[:, sy, sx].transpose(1, 2) for t in (q, k, v))  # [B, nh, 64, hd]
            logits = qw @ kw.transpose(-2, -1) * scale + table[idx].permute(2, 0, 1) + mask
            out[:, sy, sx] = (torch.softmax(logits, -1) @ vw).transpose(1, 2)
    assert (out - ref).abs().max().item() <= 1e-12
