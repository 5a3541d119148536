"""fluxmi_window_attention16 / fluxmi_channel_mean / fluxmi_channel_combine (csrc/window_attention16.hip) and modules/hat.py on the GPU.

Attention: every element within MARGIN * U_BF16 * (|ref| + A) of tests/hat_ref.py's fp64 construction, A = softmax . |v| (the attention
tests' derivation: the output's and P's bf16 rounding); |logits| stay below about 20, so the fp32 terms stay far under u.
Channel mean: a sum of P fp32 terms in any order is within (P - 1) 2^-24 sum |y| of exact, and the division rounds once more:
|mean - ref| <= MARGIN (P + 2) 2^-24 mean|y| =: dm.  Combine: relu is 1-Lipschitz and sigmoid' <= 1 / 4, so the gate moves by at most
dg = (|w2| (|w1| dm + (C + 2) 2^-24 (|w1| |mean| + |b1|)) + (Cs + 2) 2^-24 (|w2| hid + |b2|)) / 4 + 4 * 2^-24, and
|out - ref| <= MARGIN (u |ref| + s |y| dg + 4 * 2^-24 (|a| + |b| + s |y|)): the output's one bf16 rounding plus the fp32 terms.
Network: rel-L2 against fp64 <= 1.5 x that of the reference with bf16 rounding at the native rounding points (the SwinIR test's gate)."""
import ctypes as C
import importlib

import pytest
import torch

import hat_ref as hr64
import helper_refs as hr
from attention_ref import MARGIN, U_BF16
from helper_refs import bits, sentinel_like

pytestmark = pytest.mark.gpu
E32 = 2.0 ** -24
MODES = [(0, 0), (0, 8), (4, 0)]  # (overlap, shift)

ops = pytest.fixture(scope="module")(lambda: importlib.import_module("fluxmi.ops"))


def inputs(family, B, H, W, nh, hd, overlap, seed):
    """q, k, v bf16 [B, H, W, nh, hd], table fp32 [rows, nh], index int32 [256, Nk]: a random map into the table, NOT HAT's arithmetic one,
    so a kernel that recomputes the index instead of reading it fails.  "onehot": v at pixel (y, x) is the one-hot of 4 (y % 4) + x % 4, so
    column d < 16 is the softmax mass of the keys of one residue: a dropped, duplicated, misplaced or wrongly masked key is a whole element.
    Every 8 x 8 mask quadrant and every image holds all 16 residues, so no reference value is a bare exp(-100) (subnormal in fp32)."""
    g = torch.Generator().manual_seed(hr.seed_of("hat", family, B, H, W, nh, hd, overlap, seed))
    q, k, v = ((s * torch.randn(B, H, W, nh, hd, generator=g)).bfloat16() for s in (2.0, 1.0, 1.0))
    if family == "onehot":
        t = (torch.arange(H) % 4)[:, None] * 4 + (torch.arange(W) % 4)[None, :]
        v = torch.nn.functional.one_hot(t, hd).bfloat16()[None, :, :, None, :].expand(B, H, W, nh, hd).contiguous()
    rows, nk = (1521, 576) if overlap else (961, 256)
    index = (torch.randperm(256 * nk, generator=g) % rows).to(torch.int32).view(256, nk)
    return q, k, v, torch.randn(rows, nh, generator=g), index


def pack(q, k, v):  # -> the kernel's [B, H, W, 3 * nh * 32] layout, heads zero-padded to 32 columns
    B, H, W, nh, hd = q.shape
    out = torch.zeros(B, H, W, 3, nh, 32, dtype=torch.bfloat16)
    for s, t in enumerate((q, k, v)):
        out[:, :, :, s, :, :hd] = t
    return out.view(B, H, W, 3 * nh * 32)


@pytest.mark.parametrize("family", ["randn", "onehot"])
@pytest.mark.parametrize("nh", [1, 6])
@pytest.mark.parametrize("H,W", [(16, 16), (16, 48), (48, 32)])
@pytest.mark.parametrize("overlap,shift", MODES)
def test_kernel_against_fp64(ops, dev, overlap, shift, H, W, nh, family):
    B, hd = 2, 30
    scale = hd ** -0.5
    q, k, v, table, index = inputs(family, B, H, W, nh, hd, overlap, 1)
    ref, A = hr64.attention16_ref64(q, k, v, table, index, shift, overlap, scale)
    got = ops.window_attention16(pack(q, k, v).to(dev), table.to(dev), index.to(dev), nh, shift, overlap, scale).cpu().view(B, H, W, nh, 32)
    assert torch.isfinite(got).all() and not got[..., hd:].any(), "non-finite output, or a head's pad columns are not zero"
    err, bound = (got[..., :hd].double() - ref).abs(), MARGIN * U_BF16 * (ref.abs() + A)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"WINDOW_ATTN16 {H}x{W} overlap={overlap} shift={shift} heads={nh}x{hd} {family}: worst err/bound {worst:.3f} (gate 1.0)")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} elements beyond {MARGIN} u (|ref| + A); worst err/bound {worst:.3f}"


@pytest.mark.parametrize("overlap,shift", MODES)
def test_placement_frames_and_bits(ops, dev, overlap, shift):
    B, H, W, nh, hd = 2, 48, 32, 6, 30
    q, k, v, table, index = inputs("randn", B, H, W, nh, hd, overlap, 2)
    qkv, table, index, scale, Cw = pack(q, k, v).to(dev), table.to(dev), index.to(dev), hd ** -0.5, nh * 32
    run = lambda x, **kw: ops.window_attention16(x, table, index, nh, shift, overlap, scale, **kw)  # noqa: E731
    dense = run(qkv)
    ibuf, obuf = sentinel_like((B, H, W, 8 + 3 * Cw + 8), dev), sentinel_like((B, H, W, 8 + Cw + 16), dev)
    iwin, owin = ibuf[..., 8:8 + 3 * Cw], obuf[..., 8:8 + Cw]
    iwin.copy_(qkv)
    assert run(iwin, out=owin).data_ptr() == owin.data_ptr()
    for buf, n in ((ibuf, 3 * Cw), (obuf, Cw)):
        full = buf.cpu()
        assert bool((bits(full[..., :8]) == hr.SENTINEL).all() and (bits(full[..., 8 + n:]) == hr.SENTINEL).all()), "the frame lost sentinel bits"
    assert torch.equal(bits(owin), bits(dense)), "the strided windows differ from the contiguous call"
    assert torch.equal(bits(run(qkv)), bits(dense)), "two runs differ"
    assert torch.equal(bits(run(qkv[1:].contiguous())[0]), bits(dense[1])), "image 1 alone differs from image 1 in a batch of 2"


REFUSALS = {  # argument overrides of a valid call (heads 2, 16 x 32) -> a word of the refusal
    "H=24": (dict(H=24), "multiples"), "W=0": (dict(W=0), "multiples"), "shift=4": (dict(shift=4), "shift"),
    "shift with overlap": (dict(shift=8, overlap=4), "shift"), "overlap=8": (dict(overlap=8), "overlap"), "heads=0": (dict(heads=0), "heads"),
    "heads=17": (dict(heads=17), "heads"), "rows=0": (dict(rows=0), "table_rows"), "rows=1522": (dict(rows=1522), "table_rows"),
    "B=65536": (dict(B=65536), "grid"), "ld%8": (dict(ld=196), "stride"), "ld short": (dict(ld=184), "stride"), "ldo short": (dict(ldo=56), "stride"),
    "qkv unaligned": (dict(qkv_off=2), "16-byte"), "out unaligned": (dict(out_off=4), "16-byte"), "index unaligned": (dict(idx_off=4), "16-byte"),
    "overlapping": (dict(alias=True), "overlap qkv"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_before_any_launch(dev, case):
    from fluxmi import _lib

    a = dict(dict(B=1, H=16, W=32, heads=2, shift=0, overlap=0, rows=961, ld=192, ldo=64, qkv_off=0, out_off=0, idx_off=0, alias=False), **REFUSALS[case][0])
    qkv, out = torch.zeros(1, 16, 32, 192, dtype=torch.bfloat16, device=dev), sentinel_like((1, 16, 32, 64), dev)
    table, index = torch.zeros(1521, 2, device=dev), torch.zeros(256 * 576 + 4, dtype=torch.int32, device=dev)
    op = qkv.data_ptr() + 64 if a["alias"] else out.data_ptr() + a["out_off"]
    with pytest.raises(RuntimeError, match=REFUSALS[case][1]):
        _lib.call("fluxmi_window_attention16", C.c_void_p(qkv.data_ptr() + a["qkv_off"]), a["ld"], C.c_void_p(table.data_ptr()), a["rows"],
                  C.c_void_p(index.data_ptr() + a["idx_off"]), C.c_void_p(op), a["ldo"], a["B"], a["H"], a["W"], a["heads"], a["shift"], a["overlap"],
                  1.0, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((bits(out) == hr.SENTINEL).all()) and not qkv.any(), "a refused call wrote"


def test_index_outside_the_table_is_refused_on_the_host(ops, dev):
    q, k, v, table, index = inputs("randn", 1, 16, 16, 1, 30, 0, 3)
    index[7, 9] = 961
    with pytest.raises(ValueError, match="outside"):
        ops.window_attention16(pack(q, k, v).to(dev), table.to(dev), index.to(dev), 1, 0, 0, 1.0)


@pytest.mark.parametrize("Cr", [60, 180])
@pytest.mark.parametrize("H,W", [(1, 1), (16, 16), (33, 17)])
def test_channel_mean_and_combine_against_fp64(ops, dev, H, W, Cr):
    g = torch.Generator().manual_seed(hr.seed_of("cab", H, W, Cr))
    B, Cp, Cs, s, P = 2, -(-Cr // 64) * 64, Cr // 30, 0.01, H * W
    def real(*shape, std=1.0, mean=0.0):  # zero in the pad channels [Cr, Cp), as the network holds them
        t = torch.zeros(*shape, Cp)
        t[..., :Cr] = mean + std * torch.randn(*shape, Cr, generator=g)
        return t
    a, b, y = real(B, H, W).bfloat16(), real(B, H, W).bfloat16(), real(B, H, W, std=2.0, mean=0.5).bfloat16()
    w1, b1, w2, b2 = real(Cs), 0.1 * torch.randn(Cs, generator=g), real(Cs).T.contiguous(), real(mean=0.2, std=0.5)
    ref, _ = hr64.channel_combine_ref64(a, b, y, w1, b1, w2, b2, s)
    y64, w1a, w2a = y.double(), w1.double().abs(), w2.double().abs()
    mean64 = y64.mean((1, 2))
    dm = (P + 2) * E32 * y64.abs().mean((1, 2))
    pre = mean64 @ w1.double().T + b1.double()
    dhid = dm @ w1a.T + (Cp + 2) * E32 * (mean64.abs() @ w1a.T + b1.double().abs())
    dg = 0.25 * (dhid @ w2a.T + (Cs + 2) * E32 * (torch.relu(pre) @ w2a.T + b2.double().abs())) + 4 * E32
    ybuf, obuf = sentinel_like((B, H, W, 8 + Cp + 8), dev), sentinel_like((B, H, W, 16 + Cp + 8), dev)
    ywin, owin = ybuf[..., 8:8 + Cp], obuf[..., 16:16 + Cp]
    ywin.copy_(y)
    mean = ops.channel_mean(ywin)
    assert bool(((mean.cpu().double() - mean64).abs() <= MARGIN * dm).all()), "the channel mean is outside the fp32 sum's bound"
    wd = [t.to(dev) for t in (w1, b1, w2, b2)]
    got = ops.channel_combine(a.to(dev), b.to(dev), ywin, mean, *wd, s, out=owin).cpu()
    full = obuf.cpu()
    assert bool((bits(full[..., :16]) == hr.SENTINEL).all() and (bits(full[..., 16 + Cp:]) == hr.SENTINEL).all()), "the frame lost sentinel bits"
    ya = s * y64.abs()
    err, bound = (got.double() - ref).abs(), MARGIN * (U_BF16 * ref.abs() + ya * dg[:, None, None, :] + 4 * E32 * (a.double().abs() + b.double().abs() + ya))
    assert bool((err <= bound).all()), f"worst err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}"
    dense = ops.channel_combine(a.to(dev), b.to(dev), y.to(dev), ops.channel_mean(y.to(dev)), *wd, s)
    assert torch.equal(bits(dense.cpu()), bits(got)), "dense differs from strided"


@pytest.mark.parametrize("scale", [4, 2])
def test_network_against_fp64_next_to_the_bf16_model(dev, scale):
    from fluxmi import synth
    from modules.hat import HAT

    sd = synth.make_hat_state_dict(embed_dim=60, depths=(2, 2), heads=(2, 2), scale=scale, seed=5)
    net = HAT(sd, device=dev)
    x = torch.rand(2, 24, 40, 3, generator=torch.Generator().manual_seed(6)).bfloat16()
    got = net(x.to(dev))
    assert tuple(got.shape) == (2, scale * 24, scale * 40, 3) and got.dtype == torch.bfloat16 and torch.isfinite(got).all()
    assert torch.equal(bits(net(x.to(dev))), bits(got)), "two runs differ"
    ref = hr64.hat_ref(sd, x)
    rel = lambda t: float((t.double() - ref).norm() / ref.norm())  # noqa: E731
    l2_model, l2_got = rel(hr64.hat_ref(sd, x, round=hr.rbf64)), rel(got.cpu())
    print(f"HAT_PARITY x{scale} 24x40: rel-L2 bf16 model {l2_model:.3e} got {l2_got:.3e} (ratio {l2_got / l2_model:.3f}, gate 1.5)")
    assert l2_got <= 1.5 * l2_model


def test_pipeline_upscales_through_a_hat_file(dev, tmp_path):
    from test_cfg_gpu import prompts, tiny_pipeline

    from fluxmi import synth
    from modules import hat, upscaler

    torch.save(synth.make_hat_state_dict(embed_dim=60, depths=(2,), heads=(2,), scale=2, seed=7, wrap="params_ema"), tmp_path / "hat.pth")
    pipe = tiny_pipeline(dev)
    pipe.compile()
    pipe.upscaler = net = upscaler.read_upscaler(str(tmp_path / "hat.pth"), device=dev)
    assert isinstance(net, hat.HAT)
    px = torch.randint(0, 256, (2, 13, 18, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(8))
    up = pipe.upscale(px)
    assert up.dtype == torch.uint8 and tuple(up.shape) == (2, 26, 36, 3) and up.device.type == "cpu" and up.float().std() > 0
    on_dev = net.upscale_uint8_device(px)
    assert on_dev.device.type == "cuda" and on_dev.is_contiguous() and torch.equal(on_dev.cpu(), up), "upscale_uint8_device differs from upscale_uint8"
    kw = dict(width=64, height=96, num_steps=4, seed=7, silent=True, output_type="uint8")
    pos, _ = prompts()
    assert torch.equal(pipe.generate(pos, upscale=True, **kw), pipe.upscale(pipe.generate(pos, **kw))), "upscale=True differs from pipe.upscale"
