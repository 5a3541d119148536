"""The native JPEG encoder on the GPU (csrc/jpeg.hip) against tests/jpeg_ref.py, byte for byte: the case list of tests/jpeg_cases.py (whose
coverage tests/test_jpeg_cpu.py asserts), strides and sentinel frames, a too-small output, and the pipeline's jpeg_encoder="native"."""
import numpy as np
import pytest
import torch

import jpeg_cases as jc
import jpeg_ref as jr

pytestmark = pytest.mark.gpu

FRAME = 4096  # sentinel bytes before and after `work` and `out`
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ops():
    from fluxmi import ops as o

    return o


def first_difference(a: bytes, b: bytes) -> str:
    n = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return f"lengths {len(a)} / {len(b)}, first difference at byte {n}: {a[n:n + 8].hex()} / {b[n:n + 8].hex()}"


# ---- 1. byte equality ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", jc.CASES, ids=jc.case_id)
def test_encoder_equals_the_definition(ops, dev, case):
    fam, B, H, W, q, ss, R = case
    want, _ = jc.reference_of(case)
    got = ops.jpeg_encode(torch.tensor(jc.image_of(case)).to(dev), quality=q, subsampling=ss, restart_interval=R)
    assert got == want, first_difference(got, want)


@pytest.mark.parametrize("case", jc.BIG_CASES, ids=jc.case_id)
def test_thousands_of_intervals(ops, dev, case):
    fam, B, H, W, q, ss, R = case
    want, _ = jc.reference_of(case)
    assert want.count(b"\xFF\xD0") + want.count(b"\xFF\xD7") > 20
    px = torch.tensor(jc.image_of(case)).to(dev)
    got = ops.jpeg_encode(px, quality=q, subsampling=ss, restart_interval=R)
    assert got == want, first_difference(got, want)
    assert ops.jpeg_encode(px, quality=q, subsampling=ss, restart_interval=R) == got, "two runs differ"


def test_defaults(ops, dev):
    """quality 99, 4:2:0, the default interval; [H, W, 3] is refused (a batch axis is required, as for the other uint8 image entries)"""
    im = jc.make_image("photo", 2, 40, 56, seed=3)
    assert ops.jpeg_encode(torch.from_numpy(im).to(dev)) == jr.jpeg_ref(im, 99, "4:2:0", jc.DEFAULT_RESTART["4:2:0"])
    with pytest.raises(ValueError, match="B, H, W"):
        ops.jpeg_encode(torch.from_numpy(im[0]).to(dev))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.jpeg_encode(torch.from_numpy(im))


# ---- 2. robustness ------------------------------------------------------------------------------------------------------------------------
def framed(dev, n):
    buf = torch.full((n + 2 * FRAME,), SENTINEL, dtype=torch.uint8, device=dev)
    return buf, buf[FRAME:FRAME + n]


def frame_intact(buf, n) -> bool:
    return bool((buf[:FRAME] == SENTINEL).all()) and bool((buf[FRAME + n:] == SENTINEL).all())


@pytest.mark.parametrize("ss,R", [("4:2:0", None), ("4:4:4", 0), ("4:2:0", 1)])
def test_pitches_frames_and_small_outputs(ops, dev, ss, R):
    B, H, W, q = 3, 33, 41, 99
    im = jc.make_image("noise", B, H, W, seed=11)
    want = jr.jpeg_ref(im, q, ss, jc.DEFAULT_RESTART[ss] if R is None else R)
    # a row pitch above 3 W and an image pitch above H rows, random bytes in the slack
    g = torch.Generator().manual_seed(5)
    wide = torch.randint(0, 256, (B, H + 3, 3 * W + 13), dtype=torch.uint8, generator=g)
    wide[:, :H, :3 * W] = torch.from_numpy(im).reshape(B, H, 3 * W)
    px = wide.to(dev)[:, :H, :3 * W].unflatten(-1, (W, 3))
    assert px.stride() == ((H + 3) * (3 * W + 13), 3 * W + 13, 3, 1)
    nwork, cap = ops.jpeg_workspace_bytes(B, H, W, ss, R)
    assert FRAME % 256 == 0
    wbuf, work = framed(dev, nwork)
    obuf, out = framed(dev, cap)
    n = ops.jpeg_encode_into(px, work, out, q, ss, R)
    got = out[:n].cpu().numpy().tobytes()
    assert got == want, first_difference(got, want)
    assert frame_intact(wbuf, nwork) and frame_intact(obuf, cap)
    assert bool((out[n:] == SENTINEL).all()), "bytes behind the stream were written"
    # the contiguous input gives the same bytes; so does a second run
    n2 = ops.jpeg_encode_into(px.contiguous(), work, out, q, ss, R)
    assert out[:n2].cpu().numpy().tobytes() == want
    # an out that is too small: an error by name, nothing written at or beyond its end
    for small in (len(want) - 1, len(want) // 2, 700):
        obuf, out = framed(dev, small)
        with pytest.raises(RuntimeError, match="out_cap"):
            ops.jpeg_encode_into(px, work, out, q, ss, R)
        assert frame_intact(obuf, small) and frame_intact(wbuf, nwork)
        assert out.cpu().numpy().tobytes() == want[:small], "the bytes that fit are the stream's first"
    obuf, out = framed(dev, 100)  # not even the header
    with pytest.raises(RuntimeError, match="out_cap"):
        ops.jpeg_encode_into(px, work, out, q, ss, R)
    assert frame_intact(obuf, 100) and bool((out == SENTINEL).all())
    # an exact fit
    obuf, out = framed(dev, len(want))
    assert ops.jpeg_encode_into(px, work, out, q, ss, R) == len(want) and out.cpu().numpy().tobytes() == want and frame_intact(obuf, len(want))
    with pytest.raises(ValueError, match="work holds"):
        ops.jpeg_encode_into(px, work[:nwork - 256], out, q, ss, R)


# ---- 3. the pipeline ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe(dev):
    from test_cfg_gpu import tiny_pipeline

    p = tiny_pipeline(dev)
    p.compile()
    return p


@pytest.mark.parametrize("num_images", [1, 2])
def test_pipeline_native_encoder(dev, pipe, num_images):
    from test_cfg_gpu import prompts

    pos, _ = prompts()
    kw = dict(width=64, height=96, num_steps=4, seed=7, silent=True, num_images=num_images)
    px = torch.as_tensor(pipe.generate(pos, output_type="uint8", **kw))
    assert px.dtype == torch.uint8 and tuple(px.shape) == (num_images, 96, 64, 3) and px.float().std() > 0
    native = pipe.generate(pos, output_type="jpeg", jpeg_encoder="native", **kw).getvalue()
    want = jr.jpeg_ref(px.numpy(), 99, "4:2:0", jc.DEFAULT_RESTART["4:2:0"])
    assert native == want, first_difference(native, want)
    # the default request and "pil" are _jpeg's bytes on those pixels, as before
    pil = pipe._jpeg(px, 99).getvalue()
    assert pipe.generate(pos, output_type="jpeg", **kw).getvalue() == pil
    assert pipe.generate(pos, output_type="jpeg", jpeg_encoder="pil", **kw).getvalue() == pil
    # with another output type the encoder is ignored
    assert torch.equal(torch.as_tensor(pipe.generate(pos, output_type="uint8", jpeg_encoder="native", **kw)), px)
    # ... and both files decode to the same pixels: the streams differ by the restart markers alone
    import io

    from PIL import Image

    assert np.array_equal(np.asarray(Image.open(io.BytesIO(native))), np.asarray(Image.open(io.BytesIO(pil))))
    assert jr.scan_bytes(jr.jpeg_ref(px.numpy(), 99, "4:2:0", 0)) == jr.scan_bytes(pil)


def test_pipeline_native_quality_config_and_other_paths(dev, pipe):
    from test_cfg_gpu import prompts

    pos, neg = prompts()
    kw = dict(width=64, height=64, num_steps=4, seed=3, silent=True)
    px = torch.as_tensor(pipe.generate(pos, output_type="uint8", **kw)).numpy()
    assert pipe.generate(pos, jpeg_encoder="native", jpeg_quality=50, **kw).getvalue() == jr.jpeg_ref(px, 50, "4:2:0", 4)
    # the configuration's encoder is the default of a request that does not say; the request's own wins
    old = getattr(pipe.config, "jpeg_encoder", "pil")
    pipe.config.jpeg_encoder = "native"
    try:
        assert pipe.generate(pos, **kw).getvalue() == jr.jpeg_ref(px, 99, "4:2:0", 4)
        assert pipe.generate(pos, jpeg_encoder="pil", **kw).getvalue() == pipe._jpeg(torch.from_numpy(px), 99).getvalue()
    finally:
        pipe.config.jpeg_encoder = old
    # into_bytes, the tiled request and the FlowEdit request
    x = torch.rand(2, 3, 24, 40, generator=torch.Generator().manual_seed(1)).mul(2).sub(1).to(dev)
    assert pipe.into_bytes(x, 90, jpeg_encoder="native").getvalue() == jr.jpeg_ref(pipe.to_uint8(x).numpy(), 90, "4:2:0", 4)
    assert pipe.into_bytes(x, 90).getvalue() == pipe._jpeg(pipe.to_uint8(x), 90).getvalue()
    assert torch.equal(pipe.to_uint8_device(x).cpu(), pipe.to_uint8(x))
    tiled = dict(kw, width=96, height=96, tile_size=64, tile_overlap=32)
    t_px = torch.as_tensor(pipe.generate(pos, output_type="uint8", **tiled)).numpy()
    assert pipe.generate(pos, jpeg_encoder="native", **tiled).getvalue() == jr.jpeg_ref(t_px, 99, "4:2:0", 4)
    photo = torch.randint(0, 256, (64, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    edit = dict(kw, init_image=photo, source_prompt=neg, num_steps=6)
    torch.manual_seed(31)
    e_px = torch.as_tensor(pipe.generate(pos, output_type="uint8", **edit)).numpy()
    torch.manual_seed(31)
    assert pipe.generate(pos, jpeg_encoder="native", **edit).getvalue() == jr.jpeg_ref(e_px, 99, "4:2:0", 4)
    # through the upscaler: its device-returning sibling feeds the encoder what upscale() returns on the host
    from fluxmi import synth
    from modules.upscaler import RRDBNet

    assert pipe.upscaler is None
    pipe.upscaler = RRDBNet(synth.make_rrdbnet_state_dict(1, 64, 32, 4, seed=21), device=dev)
    try:
        up = torch.as_tensor(pipe.generate(pos, output_type="uint8", upscale=True, **kw))
        assert tuple(up.shape) == (1, 256, 256, 3)
        assert torch.equal(pipe.upscaler.upscale_uint8_device(torch.from_numpy(px).to(dev)).cpu(), up)
        assert pipe.generate(pos, jpeg_encoder="native", upscale=True, **kw).getvalue() == jr.jpeg_ref(up.numpy(), 99, "4:2:0", 4)
    finally:
        pipe.upscaler = None
    # refusals by name
    with pytest.raises(ValueError, match="jpeg_encoder='webp'"):
        pipe.generate(pos, jpeg_encoder="webp", **kw)
    with pytest.raises(ValueError, match="65535"):
        pipe.generate(pos, jpeg_encoder="native", **dict(kw, num_images=1024))
