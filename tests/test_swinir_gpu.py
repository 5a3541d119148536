"""fluxmi_window_attention / fluxmi_channel_norm (csrc/window_attention.hip) and modules/swinir.py on the GPU.

Attention: every element within attention_ref.MARGIN * U_BF16 * (|ref| + A) of tests/swinir_ref.py's fp64 construction, A = softmax . |v|
(the attention tests' derivation: the output's and P's bf16 rounding); |logits| stay below about 20, so the fp32 terms stay far under u.
channel_norm: |got - ref| <= MARGIN * (u |ref| + (D + 8) 2^-24 A), A = (|x - mean| + max |x|) rstd |w| + |b|: the fp32 sum of D terms moves
the mean by at most D 2^-24 max |x|, scaled by rstd |w|; the variance's D + 3 roundings move rstd by half that; four more roundings follow.
Network: rel-L2 against fp64 <= 1.5 x that of the reference with bf16 rounding at the native rounding points (the Depth Anything test's)."""
import ctypes as C
import importlib

import pytest
import torch

import helper_refs as hr
import swinir_ref as sr
from attention_ref import MARGIN, U_BF16
from helper_refs import bits, sentinel_like

pytestmark = pytest.mark.gpu

ops = pytest.fixture(scope="module")(lambda: importlib.import_module("fluxmi.ops"))


def inputs(family, B, H, W, nh, hd, shift, seed):
    """q, k, v bf16 [B, H, W, nh, hd], table fp32 [225, nh].  "onehot": v at window position (y, x) (rolled) is the one-hot of 4 (y % 4) +
    x % 4, so column d < 16 is the softmax mass of four keys, one per 4 x 4 quadrant: a misplaced or wrongly masked key is a whole element.
    One per quadrant because the shift mask leaves a query whole quadrants: every column keeps an unmasked key, and no reference value is
    a bare exp(-100) = 4e-44, which fp32 and bf16 hold only as a subnormal (a one-hot of the token index itself would ask for that)."""
    g = torch.Generator().manual_seed(hr.seed_of("swin", family, B, H, W, nh, hd, shift, seed))
    q, k, v = ((s * torch.randn(B, H, W, nh, hd, generator=g)).bfloat16() for s in (2.0, 1.0, 1.0))
    if family == "onehot":
        y, x = (torch.arange(H) - shift) % H % 4, (torch.arange(W) - shift) % W % 4
        t = y[:, None] * 4 + x[None, :]
        v = torch.nn.functional.one_hot(t, hd).bfloat16()[None, :, :, None, :].expand(B, H, W, nh, hd).contiguous()
    return q, k, v, torch.randn(225, nh, generator=g)


def pack(q, k, v):  # -> the kernel's [B, H, W, 3 * nh * 32] layout, heads zero-padded to 32 columns
    B, H, W, nh, hd = q.shape
    out = torch.zeros(B, H, W, 3, nh, 32, dtype=torch.bfloat16)
    for s, t in enumerate((q, k, v)):
        out[:, :, :, s, :, :hd] = t
    return out.view(B, H, W, 3 * nh * 32)


@pytest.mark.parametrize("family", ["randn", "onehot"])
@pytest.mark.parametrize("nh,hd", [(1, 32), (6, 30), (8, 30)])
@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("H,W", [(8, 8), (8, 16), (16, 8), (24, 16)])
def test_kernel_against_fp64(ops, dev, H, W, shift, nh, hd, family):
    B, scale = 2 if (H, W) == (24, 16) else 1, hd ** -0.5
    q, k, v, table = inputs(family, B, H, W, nh, hd, shift, 1)
    ref, A = sr.window_attention_ref64(q, k, v, table, shift, scale)
    got = ops.window_attention(pack(q, k, v).to(dev), table.to(dev), nh, shift, scale).cpu().view(B, H, W, nh, 32)
    assert torch.isfinite(got).all() and not got[..., hd:].any(), "non-finite output, or a head's pad columns are not zero"
    err, bound = (got[..., :hd].double() - ref).abs(), MARGIN * U_BF16 * (ref.abs() + A)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"WINDOW_ATTN {H}x{W} shift={shift} heads={nh}x{hd} {family}: worst err/bound {worst:.3f} (gate 1.0)")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} elements beyond {MARGIN} u (|ref| + A); worst err/bound {worst:.3f}"


@pytest.mark.parametrize("shift", [0, 4])
def test_placement_frames_and_bits(ops, dev, shift):
    B, H, W, nh, hd = 2, 24, 16, 6, 30
    q, k, v, table = inputs("randn", B, H, W, nh, hd, shift, 2)
    qkv, table, scale, Cw = pack(q, k, v).to(dev), table.to(dev), hd ** -0.5, nh * 32
    dense = ops.window_attention(qkv, table, nh, shift, scale)
    ibuf, obuf = sentinel_like((B, H, W, 8 + 3 * Cw + 8), dev), sentinel_like((B, H, W, 8 + Cw + 16), dev)
    iwin, owin = ibuf[..., 8:8 + 3 * Cw], obuf[..., 8:8 + Cw]
    iwin.copy_(qkv)
    assert ops.window_attention(iwin, table, nh, shift, scale, out=owin).data_ptr() == owin.data_ptr()
    for buf, n in ((ibuf, 3 * Cw), (obuf, Cw)):
        full = buf.cpu()
        assert bool((bits(full[..., :8]) == hr.SENTINEL).all() and (bits(full[..., 8 + n:]) == hr.SENTINEL).all()), "the frame lost sentinel bits"
    assert not dense.view(B, H, W, nh, 32)[..., hd:].any(), "pad columns are not zero"
    assert torch.equal(bits(owin), bits(dense)), "the strided windows differ from the contiguous call"
    assert torch.equal(bits(ops.window_attention(qkv, table, nh, shift, scale)), bits(dense)), "two runs differ"
    alone = ops.window_attention(qkv[:1].contiguous(), table, nh, shift, scale)
    assert torch.equal(bits(alone[0]), bits(dense[0])), "image 0 alone differs from image 0 in a batch of 2"


REFUSALS = {  # argument overrides of a valid call (heads 2, 8 x 16) -> a word of the refusal
    "H=12": (dict(H=12), "multiples"), "W=0": (dict(W=0), "multiples"), "shift=3": (dict(shift=3), "shift"),
    "heads=0": (dict(heads=0), "heads"), "heads=17": (dict(heads=17), "heads"), "B=65536": (dict(B=65536), "grid"),
    "ld%8": (dict(ld=196), "stride"), "ld short": (dict(ld=184), "stride"), "ldo short": (dict(ldo=56), "stride"),
    "qkv unaligned": (dict(qkv_off=2), "16-byte"), "out unaligned": (dict(out_off=4), "16-byte"), "overlap": (dict(alias=True), "overlap"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_before_any_launch(dev, case):
    from fluxmi import _lib

    a = dict(dict(B=1, H=8, W=16, heads=2, shift=4, ld=192, ldo=64, qkv_off=0, out_off=0, alias=False), **REFUSALS[case][0])
    qkv, out, table = torch.zeros(1, 8, 16, 192, dtype=torch.bfloat16, device=dev), sentinel_like((1, 8, 16, 64), dev), torch.zeros(225, 2, device=dev)
    op = qkv.data_ptr() + 64 if a["alias"] else out.data_ptr() + a["out_off"]
    with pytest.raises(RuntimeError, match=REFUSALS[case][1]):
        _lib.call("fluxmi_window_attention", C.c_void_p(qkv.data_ptr() + a["qkv_off"]), a["ld"], C.c_void_p(table.data_ptr()), C.c_void_p(op),
                  a["ldo"], a["B"], a["H"], a["W"], a["heads"], a["shift"], 1.0, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((bits(out) == hr.SENTINEL).all()) and not qkv.any(), "a refused call wrote"


@pytest.mark.parametrize("D,rows", [(60, 9), (180, 5), (64, 4), (3, 1)])
def test_channel_norm_against_fp64(ops, dev, D, rows):
    g = torch.Generator().manual_seed(hr.seed_of("channel_norm", D, rows))
    D8 = -(-D // 8) * 8
    x, w, b = torch.zeros(rows, D8, dtype=torch.bfloat16), torch.zeros(D8, dtype=torch.bfloat16), torch.zeros(D8, dtype=torch.bfloat16)
    x[:, :D] = (torch.randn(rows, D, generator=g) * 2 + 0.5).bfloat16()
    w[:D], b[:D] = (1 + 0.2 * torch.randn(D, generator=g)).bfloat16(), torch.randn(D, generator=g).bfloat16()
    x64, w64, b64 = x[:, :D].double(), w[:D].double(), b[:D].double()
    mean, rstd = x64.mean(1, keepdim=True), (x64.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    ref = (x64 - mean) * rstd * w64 + b64
    A = ((x64 - mean).abs() + x64.abs().amax(1, keepdim=True)) * rstd * w64.abs() + b64.abs()
    ibuf, obuf = sentinel_like((rows, 8 + D8 + 8), dev), sentinel_like((rows, 16 + D8 + 8), dev)
    ibuf[:, 8:8 + D8] = x.to(dev)
    got = ops.channel_norm(ibuf[:, 8:8 + D8], w.to(dev), b.to(dev), D, 1e-5, out=obuf[:, 16:16 + D8])
    full, got = obuf.cpu(), got.cpu()
    assert bool((bits(full[:, :16]) == hr.SENTINEL).all() and (bits(full[:, 16 + D8:]) == hr.SENTINEL).all()), "the frame lost sentinel bits"
    assert not got[:, D:].any(), "the columns [D, D8) must be zero"
    err, bound = (got[:, :D].double() - ref).abs(), MARGIN * (U_BF16 * ref.abs() + (D + 8) * 2.0 ** -24 * A)
    assert bool((err <= bound).all()), f"worst err/bound {float((err / bound).max()):.3f}"
    assert torch.equal(bits(ops.channel_norm(x.to(dev), w.to(dev), b.to(dev), D, 1e-5)[:, :D8].cpu()), bits(got)), "dense differs from strided"


CONFIGS = {"60-1conv-x4": dict(embed_dim=60, depths=(2, 2), heads=(2, 2), resi="1conv", scale=4),
           "64-3conv-x2": dict(embed_dim=64, depths=(2,), heads=(2,), resi="3conv", scale=2)}


@pytest.mark.parametrize("H,W", [(16, 24), (13, 18)])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_network_against_fp64_next_to_the_bf16_model(dev, cfg, H, W):
    from fluxmi import synth
    from modules.swinir import SwinIR

    sd = synth.make_swinir_state_dict(seed=5, **CONFIGS[cfg])
    net = SwinIR(sd, device=dev)
    x = torch.rand(2, H, W, 3, generator=torch.Generator().manual_seed(6)).bfloat16()
    got = net(x.to(dev))
    assert tuple(got.shape) == (2, net.scale * H, net.scale * W, 3) and got.dtype == torch.bfloat16 and torch.isfinite(got).all()
    assert torch.equal(bits(net(x.to(dev))), bits(got)), "two runs differ"
    ref = sr.swinir_ref(sd, x)
    rel = lambda t: float((t.double() - ref).norm() / ref.norm())  # noqa: E731
    l2_model, l2_got = rel(sr.swinir_ref(sd, x, round=hr.rbf64)), rel(got.cpu())
    print(f"SWINIR_PARITY {cfg} {H}x{W}: rel-L2 bf16 model {l2_model:.3e} got {l2_got:.3e} (ratio {l2_got / l2_model:.3f}, gate 1.5)")
    assert l2_got <= 1.5 * l2_model


def test_pipeline_upscale_through_swinir(dev):
    from test_cfg_gpu import tiny_pipeline

    from fluxmi import synth
    from modules.swinir import SwinIR

    pipe = tiny_pipeline(dev)
    pipe.upscaler = net = SwinIR(synth.make_swinir_state_dict(seed=7, **CONFIGS["60-1conv-x4"]), device=dev)
    px = torch.randint(0, 256, (2, 13, 18, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(8))
    up = pipe.upscale(px)
    assert up.dtype == torch.uint8 and tuple(up.shape) == (2, 52, 72, 3) and up.device.type == "cpu" and up.float().std() > 0
    on_dev = net.upscale_uint8_device(px)
    assert on_dev.device.type == "cuda" and on_dev.is_contiguous() and torch.equal(on_dev.cpu(), up), "upscale_uint8_device differs from upscale_uint8"
