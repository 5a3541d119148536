"""fluxmi_conv3x3_dense (csrc/upscaler.hip) on the GPU: the kernel against the fp64 reference under the per-element gate of
tests/upscaler_ref.py on a covering set of shapes, epilogue arms and sizes around its pixel tile; its bits (run to run, a sample alone
against the sample among poisoned neighbours, an in-place dense window against out of place, the folded upsample against an explicitly
repeated input, the sentinel frame around the written window); the whole RRDBNet against fp64 next to the fp32 model; the pipeline."""
import pytest
import torch

import upscaler_ref as ur
from helper_refs import bits, sentinel_like

pytestmark = pytest.mark.gpu

T = ur.TILE
PAIRS = [(16, 64), (64, 32), (96, 32), (128, 32), (160, 32), (192, 64), (64, 64), (64, 3)]  # every (Cin, Cout) of an nf 64 / gc 32 net
ARMS = {
    "none": dict(ur.ARMS_NONE),
    "bias": dict(ur.ARMS_NONE, bias=True),
    "act": dict(ur.ARMS_NONE, bias=True, act=True),
    "r1": dict(ur.ARMS_NONE, bias=True, r1=True),
    "r1r2": dict(ur.ARMS_NONE, bias=True, act=True, r1=True, r2=True),
    "up": dict(ur.ARMS_NONE, bias=True, act=True, upsample=2),
}
SIZES = [(1, 1), (2, 3), (5, 7), (T - 1, T + 1), (T, T), (T + 1, T - 1), (T + 1, T + 1), (T - 1, T), (T, T - 1)]  # OUTPUT grids


def _cases():
    """a covering set, not the cross product: every pair meets every arm at least once over two rounds of sizes, every size meets B = 1 and 3"""
    out, arms, n = [], list(ARMS), 0
    for rnd in range(len(arms)):
        for i, (cin, cout) in enumerate(PAIRS):
            arm = arms[(i + rnd) % len(arms)]
            H, W = SIZES[n % len(SIZES)]
            if arm == "up":  # an even output grid: the sizes doubled around the tile edge, or the small ones rounded up
                H, W = H + H % 2, W + W % 2
            B = 1 if (n // len(SIZES)) % 2 == 0 else 3
            fam = ur.FAMILIES[n % len(ur.FAMILIES)]
            out.append(pytest.param(cin, cout, arm, B, H, W, fam, id=f"{cin}-{cout}-{arm}-B{B}-{H}x{W}-{fam}"))
            n += 1
    return out


def pad_w(w, bias, dev):
    """w [Cout, 3, 3, Cin], bias [Cout] -> the kernel's zero-padded [Cout32, 3, 3, Cin], [Cout32]"""
    cout = w.shape[0]
    c32 = -(-cout // 32) * 32
    w2 = torch.zeros(c32, 3, 3, w.shape[-1], dtype=torch.bfloat16)
    w2[:cout] = w
    b2 = torch.zeros(c32, dtype=torch.bfloat16)
    b2[:cout] = bias
    return w2.to(dev), b2.to(dev)


def run_kernel(ops, dev, inp, arms, xbuf=None):
    """-> (out [B, H, W, Cout] on the host, frame ok): x is the window [0, Cin) of a buffer SHIFT channels wider, `out` the window
    [8, 8 + Cout) of a sentinel-filled buffer with a pixel stride 24 channels wider, the residuals windows at channel 8 of wider buffers"""
    w, up = inp["w"], arms["upsample"]
    cout, cin = w.shape[0], w.shape[-1]
    xb = (inp["xbuf"] if xbuf is None else xbuf).to(dev)
    B, Hi, Wi, _ = xb.shape
    H, W = Hi * up, Wi * up
    w2, b2 = pad_w(w, inp["bias"], dev)
    ldo = -(-cout // 8) * 8 + 24
    buf = sentinel_like((B, H, W, ldo), dev)
    out = buf[..., 8 : 8 + cout]
    res = []
    for name in ("r1", "r2"):
        if arms[name]:
            rb = torch.zeros(B, H, W, ldo, dtype=torch.bfloat16)
            rb[..., 8 : 8 + cout] = inp[name]
            res.append(rb.to(dev)[..., 8 : 8 + cout])
        else:
            res.append(None)
    got = ops.conv3x3_dense(xb[..., :cin], w2, b2 if arms["bias"] else None, out, r1=res[0], a1=ur.A1, r2=res[1], a2=ur.A2, slope=ur.SLOPE,
                            act=arms["act"], upsample=up)
    assert got.data_ptr() == out.data_ptr()
    full = buf.cpu()
    frame = full.clone()
    frame[..., 8 : 8 + cout] = sentinel_like((B, H, W, cout))
    return full[..., 8 : 8 + cout].contiguous(), bool((bits(frame) == bits(sentinel_like(frame.shape))).all())


@pytest.fixture(scope="module")
def ops():
    from fluxmi import ops as o

    return o


@pytest.mark.parametrize("cin,cout,arm,B,H,W,fam", _cases())
def test_kernel_against_the_gate(ops, dev, cin, cout, arm, B, H, W, fam):
    arms = ARMS[arm]
    up = arms["upsample"]
    inp = ur.conv_inputs(fam, B, H // up, W // up, cin, cout, seed=5, upsample=up)
    got, frame_ok = run_kernel(ops, dev, inp, arms)
    n_bad, worst = ur.conv_check(got, ur.conv_gate(inp, arms))
    print(f"CONV_DENSE_BOUND {cin}->{cout} {arm} B={B} {H}x{W} {fam}: worst err/bound {worst:.3f} (gate {ur.MARGIN})")
    assert n_bad == 0, f"{n_bad} elements beyond {ur.MARGIN} x the bound; worst err/bound {worst:.3f}"
    assert frame_ok, "a channel outside the written window, or a pixel-stride gap, lost its sentinel bits"


@pytest.mark.parametrize("cin,cout", [(64, 32), (192, 64), (64, 3)])
def test_bits_run_to_run_and_sample_among_poison(ops, dev, cin, cout):
    arms = ARMS["r1r2"]
    inp = ur.conv_inputs("randn", 3, T + 1, T + 1, cin, cout, seed=6)
    a, _ = run_kernel(ops, dev, inp, arms)
    a2, _ = run_kernel(ops, dev, inp, arms)
    assert torch.equal(bits(a), bits(a2)), "two runs differ"
    one = {k: (v[1:2] if k in ("xbuf", "r1", "r2") else v) for k, v in inp.items()}
    alone, _ = run_kernel(ops, dev, one, arms)
    pois = dict(inp)
    sign = torch.where(torch.arange(inp["xbuf"][0].numel()).reshape(inp["xbuf"][0].shape) % 3 == 0, -1.0e4, 1.0e4).bfloat16()
    pois["xbuf"] = torch.stack((sign, inp["xbuf"][1], sign))
    among, _ = run_kernel(ops, dev, pois, arms)
    assert torch.equal(bits(alone[0]), bits(a[1])), "sample 1 alone differs from the same sample inside B = 3"
    assert torch.equal(bits(among[1]), bits(a[1])), "sample 1 changed with +-1e4 neighbours in the batch"


@pytest.mark.parametrize("cin,cout", [(64, 32), (160, 32)])
def test_in_place_dense_window_equals_out_of_place(ops, dev, cin, cout):
    arms = ARMS["act"]
    inp = ur.conv_inputs("randn", 2, T + 1, 5, cin, cout, seed=7)
    ref, _ = run_kernel(ops, dev, inp, arms)
    B, H, W, _ = inp["xbuf"].shape
    buf = sentinel_like((B, H, W, cin + cout + 8), dev)
    buf[..., :cin] = inp["xbuf"][..., :cin].to(dev)
    w2, b2 = pad_w(inp["w"], inp["bias"], dev)
    ops.conv3x3_dense(buf[..., :cin], w2, b2, buf[..., cin : cin + cout], slope=ur.SLOPE, act=True)
    res = buf.cpu()
    assert torch.equal(bits(res[..., cin : cin + cout]), bits(ref)), "the in-place window differs from the out-of-place launch"
    assert torch.equal(bits(res[..., :cin]), bits(inp["xbuf"][..., :cin])), "the input window was written"
    assert bool((bits(res[..., cin + cout :]) == bits(sentinel_like((B, H, W, 8)))).all()), "the channels behind the window were written"


@pytest.mark.parametrize("cin,cout,Hi,Wi", [(64, 64, T // 2, T // 2 + 1), (64, 32, 3, T)])
def test_folded_upsample_equals_repeated_input(ops, dev, cin, cout, Hi, Wi):
    inp = ur.conv_inputs("randn", 2, Hi, Wi, cin, cout, seed=8, upsample=2)
    folded, ok = run_kernel(ops, dev, inp, ARMS["up"])
    rep = inp["xbuf"].repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    plain, _ = run_kernel(ops, dev, inp, ARMS["act"], xbuf=rep)
    assert ok and torch.equal(bits(folded), bits(plain)), "upsample = 2 differs from the same launch on a repeated input"


def test_refusals_name_the_limit(ops, dev):
    x = torch.zeros(1, 4, 4, 64, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(32, 3, 3, 64, dtype=torch.bfloat16, device=dev)
    out = torch.zeros(1, 4, 4, 32, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match="Cin"):
        ops.conv3x3_dense(x[..., :24], torch.zeros(32, 3, 3, 24, dtype=torch.bfloat16, device=dev), None, out)
    with pytest.raises(RuntimeError, match="16-byte"):
        ops.conv3x3_dense(x[..., :32], torch.zeros(32, 3, 3, 32, dtype=torch.bfloat16, device=dev), None, x[..., 36:60])
    with pytest.raises(RuntimeError, match="r2"):
        ops.conv3x3_dense(x, w, None, out, r2=torch.zeros_like(out))
    with pytest.raises(RuntimeError, match="overlap"):
        ops.conv3x3_dense(x, w, None, out, r1=out)
    with pytest.raises(ValueError):
        ops.conv3x3_dense(x, w, None, out.permute(0, 2, 1, 3))


# ---- the whole network ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["new", "old"])
@pytest.mark.parametrize("num_block", [1, 2])
def test_network_against_fp64_next_to_the_model(dev, num_block, layout):
    """rel-L2 against fp64 within 1.25 x the fp32 model's, max abs error within 1.5 x the model's (two fp32 summation orders of the model
    differ from each other by up to 1.006 / 1.16 in these figures on the CPU)"""
    from fluxmi import synth
    from modules.upscaler import RRDBNet, normalize_state_dict

    sd = synth.make_rrdbnet_state_dict(num_block, 64, 32, 4, seed=11, layout=layout)
    net = RRDBNet(sd, device=dev)
    assert (net.num_block, net.nf, net.gc, net.scale, net.layout) == (num_block, 64, 32, 4, layout)
    x = torch.rand(2, 20, 24, 3, generator=torch.Generator().manual_seed(12)).bfloat16()
    got = net(x.to(dev))
    assert tuple(got.shape) == (2, 80, 96, 3) and got.dtype == torch.bfloat16
    assert torch.equal(bits(net(x.to(dev)).cpu()), bits(got.cpu())), "two runs differ"
    new, _ = normalize_state_dict(sd)
    ref = ur.net_ref64(new, x)
    l2_m, mx_m = ur.net_figures(ur.net_model(new, x), ref)
    l2_g, mx_g = ur.net_figures(got.float(), ref)
    print(f"RRDBNET_PARITY blocks={num_block} {layout}: rel-L2 model {l2_m:.3e} got {l2_g:.3e} (ratio {l2_g / l2_m:.3f}, gate 1.25); "
          f"max abs model {mx_m:.3e} got {mx_g:.3e} (ratio {mx_g / mx_m:.3f}, gate 1.5); |ref| max {ref.abs().max().item():.2f}")
    assert l2_g <= 1.25 * l2_m and mx_g <= 1.5 * mx_m


def test_uint8_value_range(dev):
    from fluxmi import synth
    from modules.upscaler import RRDBNet

    net = RRDBNet(synth.make_rrdbnet_state_dict(1, 64, 32, 4, seed=11), device=dev)
    px = torch.randint(0, 256, (2, 9, 7, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    out = net.upscale_uint8(px)
    y = net(px.to(dev).float().div(255.0).bfloat16()).float().cpu()
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2, 36, 28, 3) and out.device.type == "cpu"
    assert torch.equal(out, y.clamp(0, 1).mul(255.0).round().to(torch.uint8))


@pytest.mark.parametrize("scale", [2, 1])
def test_unshuffle_heads_run(dev, scale):
    """x2 / x1: Real-ESRGAN's pixel_unshuffle in front of the same trunk, against the reference on the unshuffled input"""
    from fluxmi import synth
    from modules.upscaler import RRDBNet

    sd = synth.make_rrdbnet_state_dict(1, 64, 32, scale, seed=13)
    net = RRDBNet(sd, device=dev)
    x = torch.rand(1, 16, 24, 3, generator=torch.Generator().manual_seed(14)).bfloat16()
    got = net(x.to(dev))
    assert tuple(got.shape) == (1, 16 * scale, 24 * scale, 3)
    u = 4 // scale
    xu = torch.nn.functional.pixel_unshuffle(x.float().permute(0, 3, 1, 2), u).permute(0, 2, 3, 1)
    ref = ur.net_ref64(sd, xu)
    l2_m, mx_m = ur.net_figures(ur.net_model(sd, xu), ref)
    l2_g, mx_g = ur.net_figures(got.float(), ref)
    print(f"RRDBNET_PARITY x{scale}: rel-L2 model {l2_m:.3e} got {l2_g:.3e}; max abs model {mx_m:.3e} got {mx_g:.3e}")
    assert l2_g <= 1.25 * l2_m and mx_g <= 1.5 * mx_m


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe(dev):
    from test_cfg_gpu import tiny_pipeline

    from fluxmi import synth
    from modules.upscaler import RRDBNet

    p = tiny_pipeline(dev)
    p.compile()
    assert p.model.calibration_state()[0] and p.upscaler is None
    p.upscaler = RRDBNet(synth.make_rrdbnet_state_dict(1, 64, 32, 4, seed=21), device=dev)
    return p


def test_pipeline_upscale_after_generation(dev, pipe):
    from test_cfg_gpu import prompts

    pos, _ = prompts()
    kw = dict(width=64, height=96, num_steps=4, seed=7, silent=True, output_type="uint8")
    plain = pipe.generate(pos, **kw)
    up = pipe.generate(pos, upscale=True, **kw)
    s = pipe.upscaler.scale
    assert plain.dtype == torch.uint8 and tuple(plain.shape) == (1, 96, 64, 3) and tuple(up.shape) == (1, 96 * s, 64 * s, 3)
    assert torch.equal(up, pipe.upscale(plain)), "upscale=True differs from pipe.upscale of the plain request's pixels"
    assert up.float().std() > 0
    # configured but not requested == a pipeline without one
    net, pipe.upscaler = pipe.upscaler, None
    try:
        without = pipe.generate(pos, **kw)
        with pytest.raises(ValueError, match="upscaler_path"):
            pipe.generate(pos, upscale=True, **kw)
    finally:
        pipe.upscaler = net
    assert torch.equal(without, plain), "a configured upscaler changed a request that did not ask for it"
    # a tiled request returns pixels too; JPEG output decodes at the larger size
    tiled = dict(kw, width=96, height=96, tile_size=64, tile_overlap=32)
    t_up = pipe.generate(pos, upscale=True, **tiled)
    assert torch.equal(t_up, pipe.upscale(pipe.generate(pos, **tiled)))
    from PIL import Image

    jpg = pipe.generate(pos, upscale=True, **dict(kw, output_type="jpeg"))
    assert Image.open(jpg).size == (64 * s, 96 * s)


def test_pipeline_init_upscale_before_img2img(dev, pipe):
    from test_cfg_gpu import prompts

    pos, _ = prompts()
    photo = torch.randint(0, 256, (24, 16, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    kw = dict(width=64, height=96, num_steps=6, seed=9, strength=0.6, silent=True, output_type="latent")
    # the VAE's encode samples its posterior from torch's global generator (the reference's randn_like): seed it before every request
    torch.manual_seed(31)
    a = pipe.generate(pos, init_image=photo, init_upscale=True, **kw)
    big = pipe.upscale(photo)
    assert tuple(big.shape) == (1, 96, 64, 3)
    torch.manual_seed(31)
    b = pipe.generate(pos, init_image=big[0], **kw)
    assert torch.equal(a, b), "init_upscale=True differs from passing the pre-upscaled image"
    torch.manual_seed(31)
    assert not torch.equal(a, pipe.generate(pos, init_image=photo, **kw)), "the network changed nothing: the result equals the plain resize's"
