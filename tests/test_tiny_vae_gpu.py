"""The tiny autoencoder on the GPU: fluxmi_conv3x3_block (csrc/tiny_vae.hip) bit for bit on integer data and under a per-element bound on
random data, its refusals, the decoder module next to its own bf16 restatement, fluxmi_latent_preview_x0, and the pipeline's decoder="tiny"."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import preview_ref as pr
from helper_refs import bits, sentinel_like

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 3, 5), (2, 16, 16), (1, 17, 33), (2, 40, 24)]  # a pixel, below a tile, one tile, one past it on each axis, several


def block_ref(x, w, b):
    """fp64, unrounded intermediates: x [B, H, W, 64], w [3, 64, 3, 3, 64] (conv, cout, dy, dx, cin), b [3, 64] -> (out, m1, m2, y)"""
    conv = lambda t, i: F.conv2d(t, w[i].double().permute(0, 3, 1, 2), b[i].double(), padding=1)
    t = x.double().permute(0, 3, 1, 2)
    m1 = F.relu(conv(t, 0))
    m2 = F.relu(conv(m1, 1))
    y = conv(m2, 2) + t
    return F.relu(y).permute(0, 2, 3, 1), m1, m2, y


def run_block(dev, x, w, b, ldx=64, ldo=64):
    """-> (out on the host, whether everything around the written window kept its sentinel bits)"""
    from fluxmi import ops

    B, H, W, _ = x.shape
    xb = torch.zeros(B, H, W, ldx, dtype=torch.bfloat16)
    xb[..., :64] = x
    buf = sentinel_like((B, H, W, ldo), dev)
    off = 8 if ldo > 64 else 0
    ops.conv3x3_block(xb.to(dev)[..., :64], w.bfloat16().to(dev), b.bfloat16().to(dev), buf[..., off:off + 64])
    full = buf.cpu()
    frame = full.clone()
    frame[..., off:off + 64] = sentinel_like((B, H, W, 64))
    return full[..., off:off + 64].float(), bool((bits(frame) == bits(sentinel_like(frame.shape))).all())


@pytest.mark.parametrize("B,H,W,ldx,ldo", [s + (64, 64) for s in SHAPES] + [(1, 17, 33, 72, 88)])
def test_block_exact_on_integers(dev, B, H, W, ldx, ldo):
    """x in -2..2, biases in {-1, 0, 1}, four +-1 weights per output channel: every value is an integer below 256, so bf16 and fp32 are exact"""
    g = torch.Generator().manual_seed(B * 10000 + H * 100 + W)
    x = torch.randint(-2, 3, (B, H, W, 64), generator=g).float()
    b = torch.randint(-1, 2, (3, 64), generator=g).float()
    w = torch.zeros(3 * 64, 9 * 64)
    w.scatter_(1, torch.rand(3 * 64, 9 * 64, generator=g).topk(4, dim=1).indices, torch.randint(0, 2, (3 * 64, 4), generator=g).float() * 2 - 1)
    w = w.reshape(3, 64, 3, 3, 64)
    ref, m1, m2, y = block_ref(x, w, b)
    assert m1.abs().max() <= 9 and m2.abs().max() <= 37 and y.abs().max() <= 151
    got, frame_ok = run_block(dev, x, w, b, ldx, ldo)
    assert torch.equal(got.double(), ref), f"{int((got.double() != ref).sum())} of {ref.numel()} values differ"
    assert frame_ok, "a channel outside the written window lost its sentinel bits"


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_block_random_within_the_rounding_bound(dev, B, H, W):
    """|out - ref| <= 1.25 * 3 * 2^-9 * A3: three bf16 roundings of half an ulp through 1-Lipschitz ReLUs, A3 the block on absolute values"""
    g = torch.Generator().manual_seed(7 + H)
    x = torch.randn(B, H, W, 64, generator=g).bfloat16().float()
    w = (torch.randn(3, 64, 3, 3, 64, generator=g) * (1.4 / 24)).bfloat16().float()
    b = (0.1 * torch.randn(3, 64, generator=g)).bfloat16().float()
    ref = block_ref(x, w, b)[0]
    a3 = block_ref(x.abs(), w.abs(), b.abs())[0]
    got, _ = run_block(dev, x, w, b)
    ratio = ((got.double() - ref).abs() / (3 * 2.0 ** -9 * a3)).max().item()
    print(f"CONV_BLOCK_BOUND B={B} {H}x{W}: worst err/bound {ratio:.3f} (gate 1.25)")
    assert ratio <= 1.25


@pytest.mark.parametrize("what,match", [("B0", "B=0"), ("H0", "H=0"), ("W0", "W=0"), ("gridB", "65535"), ("gridH", "65535"), ("ldx8", "ldx"),
                                        ("ldx_short", "ldx"), ("ldo8", "ldo"), ("align", "16-byte"), ("overlap", "overlap"), ("null", "NULL")])
def test_block_refusals_come_before_any_launch(dev, what, match):
    from fluxmi import _lib

    x = torch.zeros(1, 4, 4, 64, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(3, 64, 3, 3, 64, dtype=torch.bfloat16, device=dev)
    b = torch.zeros(3, 64, dtype=torch.bfloat16, device=dev)
    out = sentinel_like((1, 4, 4, 64), dev)
    a = dict(x=x.data_ptr(), ldx=64, w=w.data_ptr(), bias=b.data_ptr(), out=out.data_ptr(), ldo=64, B=1, H=4, W=4)
    a.update({"B0": dict(B=0), "H0": dict(H=0), "W0": dict(W=0), "gridB": dict(B=65536), "gridH": dict(H=16 * 65535 + 1), "ldx8": dict(ldx=68),
              "ldx_short": dict(ldx=56), "ldo8": dict(ldo=76), "align": dict(x=x.data_ptr() + 8), "overlap": dict(out=x.data_ptr() + 64),
              "null": dict(bias=None)}[what])
    rc = _lib.lib.fluxmi_conv3x3_block(*(a[k] for k in ("x", "ldx", "w", "bias", "out", "ldo", "B", "H", "W")), None)
    assert rc != 0 and match in _lib.lib.fluxmi_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(bits(out.cpu()), bits(sentinel_like((1, 4, 4, 64)))) and not x.any()


# ---- the decoder module ------------------------------------------------------------------------------------------------------------------
def decoder_ref(sd, z, scale, shift, rnd):
    """the docstring of modules/tiny_vae.py in fp64; rnd = what happens where the native module rounds to bf16 (identity: the reference)"""
    conv = lambda t, k: F.conv2d(t, sd[k + ".weight"].double(), sd[k + ".bias"].double() if k + ".bias" in sd else None, padding=1)
    x = rnd(3 * torch.tanh((z.double() / scale + shift) / 3))
    x = rnd(F.relu(conv(x, "1")))
    for i in range(3, 19):
        if i in (6, 11, 16):
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        elif i in (7, 12, 17):
            x = rnd(conv(x, str(i)))
        else:
            m = rnd(F.relu(conv(rnd(F.relu(conv(x, f"{i}.conv.0"))), f"{i}.conv.2")))
            x = rnd(F.relu(conv(m, f"{i}.conv.4") + x))
    return 2 * rnd(conv(x, "19")) - 1


@pytest.mark.parametrize("h,w", [(5, 7), (16, 16)])
def test_decoder_next_to_its_bf16_restatement(dev, h, w):
    from fluxmi import synth
    from modules.tiny_vae import TinyDecoder

    sd = synth.make_taef1_state_dict(seed=5)
    net = TinyDecoder(synth.make_taef1_state_dict(seed=5, prefix="decoder.layers."), device=dev, scale_factor=0.3611, shift_factor=0.1159)
    z = torch.randn(2, 16, h, w, generator=torch.Generator().manual_seed(h)).bfloat16().float()
    got = net.decode(z.to(dev)).cpu().double()
    assert tuple(got.shape) == (2, 3, 8 * h, 8 * w) and torch.equal(net.decode(z.to(dev)).cpu().double(), got)
    ref = decoder_ref(sd, z, 0.3611, 0.1159, lambda t: t)
    model = decoder_ref(sd, z, 0.3611, 0.1159, lambda t: t.bfloat16().double())
    l2 = lambda a: ((a - ref).norm() / ref.norm()).item()
    print(f"TINY_AE_PARITY {h}x{w}: rel-L2 bf16 restatement {l2(model):.3e}, native {l2(got):.3e} (ratio {l2(got) / l2(model):.3f}, gate 1.25); "
          f"y std {((ref + 1) / 2).std().item():.3f}")
    assert l2(got) <= 1.25 * l2(model)


# ---- fluxmi_latent_preview_x0 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guided", [False, True])
def test_preview_x0_keeps_the_rgb_and_stores_the_estimate(dev, guided):
    from fluxmi import _lib, ops

    B, grid, step = 2, (5, 7), 4  # 35 tokens; ctl (2, 0): slot (4 / 2) % SLOTS = 2
    x, pred, proj, t, s = pr.draws(B, grid, seed=3, guided=guided, img_rows=40, c_in=72)
    dv = lambda a: torch.from_numpy(a).to(dev).bfloat16()
    ts = torch.full((8,), float(t), dtype=torch.float32, device=dev)
    kw = dict(scale=float(s) if guided else None, step=step, ctl=(2, 0))
    rgb = ops.latent_preview(dv(x), dv(pred), ts, list(proj), grid, **kw)
    ring = sentinel_like((_lib.PREVIEW_SLOTS, B, 35, 64), dev)
    rgb2 = ops.latent_preview(dv(x), dv(pred), ts, list(proj), grid, x0_out=ring, **kw)
    assert torch.equal(rgb2, rgb) and rgb[2].any()
    f32, f64 = np.float32, np.float64
    fma = lambda a, b, d: (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(d, f64)).astype(f32)
    c, u = pred[:B], pred[B:]
    v = fma(f32(s), (c - u).astype(f32), u) if guided else c
    want = torch.from_numpy(pr.bf16_round(fma(-f32(t), v, x[:B, :35, :64]))).bfloat16()
    got = ring.cpu()
    assert torch.equal(bits(got[2]), bits(want)), "the written slot is not bf16 of the fp32 estimate"
    assert torch.equal(bits(got[:2]), bits(sentinel_like((2, B, 35, 64)))), "another slot was written"


# ---- the pipeline --------------------------------------------------------------------------------------------------------------------------
def test_pipeline_tiny_decoder(dev):
    from test_cfg_gpu import prompts, tiny_pipeline

    from fluxmi import synth
    from modules.tiny_vae import TinyDecoder

    pipe = tiny_pipeline(dev)
    pipe.compile()
    pos, _ = prompts()
    kw = dict(width=64, height=96, num_steps=4, seed=7, silent=True)
    plain = pipe.generate(pos, output_type="uint8", **kw)
    with pytest.raises(ValueError, match="tiny_ae_path"):
        pipe.generate(pos, output_type="uint8", decoder="tiny", **kw)
    ae = pipe.config.ae_params
    pipe.tiny_ae = TinyDecoder(synth.make_taef1_state_dict(seed=5), device=dev, scale_factor=ae.scale_factor, shift_factor=ae.shift_factor)
    assert torch.equal(pipe.generate(pos, output_type="uint8", **kw), plain), "a configured tiny decoder changed a request that did not ask for it"
    lat = pipe.generate(pos, output_type="latent", **kw)
    tiny = pipe.generate(pos, output_type="uint8", decoder="tiny", **kw)
    assert tuple(tiny.shape) == (1, 96, 64, 3) and tiny.float().std() > 0 and not torch.equal(tiny, plain)
    assert torch.equal(tiny, pipe.to_uint8(pipe.tiny_decode(lat)))
    from PIL import Image

    png = pipe.generate(pos, output_type="png", decoder="tiny", **kw)
    assert torch.equal(torch.from_numpy(np.array(Image.open(png))), tiny[0])
    tiled = dict(kw, width=96, height=96, tile_size=64, tile_overlap=32)
    t_lat = pipe.generate(pos, output_type="latent", **tiled)
    assert torch.equal(pipe.generate(pos, output_type="uint8", decoder="tiny", **tiled), pipe.to_uint8(pipe.tiny_decode(t_lat)))
    # previews through the tiny decoder: full-resolution uint8 at the right evaluations, the latents untouched, and one more graph kind
    # that a request without the option never captures
    kw2 = dict(kw, num_images=2, output_type="latent")
    lat2 = pipe.generate(pos, **kw2)
    seen, proj = [], []
    pipe.generate(pos, on_step=lambda info: proj.append(info["preview"]), preview_every=2, **kw2)
    cap0 = pipe.model.preview_stats()[0]
    assert torch.equal(pipe.generate(pos, on_step=lambda info: proj.append(info["preview"]), preview_every=2, **kw2), lat2)
    assert pipe.model.preview_stats()[0] == cap0, "a latent-preview request captured again"
    got = pipe.generate(pos, on_step=lambda info: seen.append((info["evaluation"], info["preview"])), preview_every=2, preview_decoder="tiny", **kw2)
    assert torch.equal(got, lat2), "tiny previews changed the latents"
    assert [e for e, _ in seen] == [0, 1, 2, 3] and all((pv is None) == (e % 2 == 1) for e, pv in seen)
    for _, pv in seen[::2]:
        assert pv.shape == (2, 96, 64, 3) and pv.dtype == np.uint8 and pv.std() > 0
    assert not np.array_equal(seen[0][1], seen[2][1])
    from fluxmi import _lib, ops

    ring = torch.empty(_lib.PREVIEW_SLOTS, 2, 24, 64, dtype=torch.bfloat16, device=dev)  # evaluations 0 and 2 sit in slots 0 and 1
    _lib.call("fluxmi_engine_copy_buffer", pipe.model._engine, b"preview_x0", 0, ops._p(ring), ring.numel() * 2, 0, ops._stream())
    for e, slot in ((0, 0), (2, 1)):
        want = pipe.to_uint8(pipe.tiny_decode(pipe.unpack(ring[slot].float(), 96, 64))).numpy()
        assert np.array_equal(seen[e][1], want), f"the preview of evaluation {e} is not the tiny decode of ring slot {slot}"
    tiny_kw = dict(kw2, on_step=lambda info: True, preview_every=2, preview_decoder="tiny")
    pipe.generate(pos, **tiny_kw)
    cap1 = pipe.model.preview_stats()[0]
    assert cap1 > cap0, "keeping the estimate is a graph kind of its own"
    assert torch.equal(pipe.generate(pos, **tiny_kw), lat2) and pipe.model.preview_stats()[0] == cap1
    for _ in range(2):  # back to latent previews: the switch captures what the switch to tiny did, and then nothing more
        assert torch.equal(pipe.generate(pos, on_step=lambda info: proj.append(info["preview"]), preview_every=2, **kw2), lat2)
    cap2 = pipe.model.preview_stats()[0]
    assert cap2 - cap1 == cap1 - cap0
    pipe.generate(pos, on_step=lambda info: True, preview_every=2, **kw2)
    assert pipe.model.preview_stats()[0] == cap2, "a request without preview_decoder captured again"
    assert proj[0].shape == (2, 12, 8, 3)
