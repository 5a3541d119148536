"""HAT without a GPU: read_upscaler's dispatch, the loader's refusals by name (modules/hat.py), and tests/hat_ref.py's nn.Unfold construction
of the overlapping keys against a direct loop over windows and key pixels."""
import pytest
import torch

import hat_ref as hr64

TINY = dict(embed_dim=60, depths=(2, 2), heads=(2, 2), scale=4)


def test_read_upscaler_dispatches_by_keys(tmp_path):
    from fluxmi import synth
    from modules import hat, swinir, upscaler

    torch.save(synth.make_hat_state_dict(seed=1, wrap="params_ema", **TINY), tmp_path / "hat.pth")
    torch.save(synth.make_swinir_state_dict(seed=2, wrap="params"), tmp_path / "swin.pth")
    torch.save(synth.make_rrdbnet_state_dict(1, 64, 32, 4, seed=2), tmp_path / "rrdb.pth")
    net = upscaler.read_upscaler(str(tmp_path / "hat.pth"), device="cpu")
    assert isinstance(net, hat.HAT) and net.scale == 4 and (net.C, net.Cp, net.Cm) == (60, 64, 32)
    g = net.geometry
    assert (g["depths"], g["heads"], g["mlp_hidden"], g["ocab_hidden"], g["compress"], g["squeeze"], g["num_feat"]) == ([2, 2], [2, 2], 120, 120, 20, 2, 64)
    assert isinstance(upscaler.read_upscaler(str(tmp_path / "swin.pth"), device="cpu"), swinir.SwinIR)
    assert isinstance(upscaler.read_upscaler(str(tmp_path / "rrdb.pth"), device="cpu"), upscaler.RRDBNet)


def test_computed_indices_serve_a_file_without_buffers():
    from fluxmi import synth
    from modules import hat

    a, b = (hat.HAT(synth.make_hat_state_dict(seed=1, with_index=w, **TINY), device="cpu") for w in (True, False))
    assert torch.equal(a.index_sa, b.index_sa) and torch.equal(a.index_oca, b.index_oca)
    assert int(a.index_oca.min()) >= 0 and int(a.index_oca.max()) < hat.OCA_ROWS and a.index_oca.dtype == torch.int32


G0, Z = "layers.0.residual_group.", torch.zeros(1)
VARIANTS = {  # the word the refusal must hold -> (synth arguments, keys added to the checkpoint, key prefixes dropped from it)
    "x3": ({}, {"upsample.0.weight": torch.zeros(576, 64, 3, 3)}, ()), "x8": ({}, {"upsample.4.weight": Z}, ()),
    "window 8": ({}, {G0 + "blocks.0.attn.relative_position_bias_table": torch.zeros(225, 2)}, ()),
    "overlap ratio of 0.25": ({}, {G0 + "overlap_attn.relative_position_bias_table": torch.zeros(35 * 35, 2)}, ()),
    "3conv": ({}, {"layers.0.conv.0.weight": Z}, ("layers.0.conv.",)), "ape": ({}, {"absolute_pos_embed": Z}, ()),
    "head_dim": (dict(heads=(1, 1)), {}, ()), "C > 256": (dict(embed_dim=288, depths=(1,), heads=(9,)), {}, ()),
    "outside": ({}, {"relative_position_index_SA": torch.full((256, 256), 961)}, ()),
    "unexpected key": ({}, {"conv_extra.weight": Z}, ()), "expected": ({}, {G0 + "overlap_attn.proj.weight": torch.zeros(60, 30)}, ()),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_refused_by_name(name):
    from fluxmi import synth
    from modules import hat
    from modules.upscaler import UpscalerFormatError

    args, add, drop = VARIANTS[name]
    sd = {k: v for k, v in synth.make_hat_state_dict(seed=3, **{**TINY, **args}).items() if not k.startswith(drop or ("\0",))}
    with pytest.raises(UpscalerFormatError, match=name):
        hat.HAT({**sd, **add}, device="cpu")


@pytest.mark.parametrize("H,W", [(16, 16), (32, 48)])
def test_unfold_construction_equals_a_loop_over_windows(H, W):
    """per window: softmax(q k^T scale + table[index]) v over the 24 x 24 pixels from (16 wy - 4, 16 wx - 4), zero k / v outside the image"""
    g = torch.Generator().manual_seed(H * 100 + W)
    B, nh, hd, scale = 2, 3, 5, 0.4
    q, k, v = (torch.randn(B, H, W, nh, hd, generator=g, dtype=torch.float64) for _ in range(3))
    table = torch.randn(1521, nh, generator=g, dtype=torch.float64)
    index = torch.randint(0, 1521, (256, 576), generator=g)
    ref, _ = hr64.attention16_ref64(q, k, v, table, index, 0, 4, scale)
    bias, out = table[index].permute(2, 0, 1), torch.empty_like(ref)
    for wy in range(H // 16):
        for wx in range(W // 16):
            kw, vw = torch.zeros(B, 24, 24, nh, hd, dtype=torch.float64), torch.zeros(B, 24, 24, nh, hd, dtype=torch.float64)
            for ky in range(24):
                for kx in range(24):
                    y, x = 16 * wy - 4 + ky, 16 * wx - 4 + kx
                    if 0 <= y < H and 0 <= x < W:
                        kw[:, ky, kx], vw[:, ky, kx] = k[:, y, x], v[:, y, x]
            qw = q[:, 16 * wy:16 * wy + 16, 16 * wx:16 * wx + 16].reshape(B, 256, nh, hd).transpose(1, 2)
            logits = qw @ kw.view(B, 576, nh, hd).permute(0, 2, 3, 1) * scale + bias
            o = torch.softmax(logits, -1) @ vw.view(B, 576, nh, hd).transpose(1, 2)
            out[:, 16 * wy:16 * wy + 16, 16 * wx:16 * wx + 16] = o.transpose(1, 2).reshape(B, 16, 16, nh, hd)
    assert (out - ref).abs().max().item() <= 1e-12
