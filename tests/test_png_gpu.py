"""The native PNG encoder on the GPU (csrc/png.hip): every file decodes (Pillow: chunk CRCs; zlib: Adler-32) to exactly the pixels, its
filtered scanlines are tests/png_ref.py's, its size respects the definition's bound, and the pipeline's output_type="png" returns it."""
import io
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import png_ref as pr

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ops():
    from fluxmi import ops as o

    return o


def content(kind: str, B: int, H: int, W: int, C: int) -> np.ndarray:
    rng = np.random.default_rng(B * 1000003 + H * 1009 + W * 7 + C)
    shape = (B, H, W, C)
    if kind == "noise":
        px = rng.integers(0, 256, shape)
    elif kind == "zeros":
        px = np.zeros(shape)
    elif kind == "single":
        px = np.zeros(shape)
        px[B - 1, H // 2, W // 2, C - 1] = 200
    elif kind == "runs":  # every row starts with runs of n equal bytes, n - 1 = 2, 3, 258 .. 261 (1049 bytes), each behind a different byte
        lens = np.tile([3, 4, 259, 260, 261, 262], W * C // 1049 + 1)
        px = np.stack([np.repeat((np.arange(len(lens)) * 37 + 11 * y) % 251 + 1, lens)[:W * C] for y in range(B * H)]).reshape(shape)
    elif kind == "flat":  # flat regions and ramps
        y, x = np.mgrid[0:B * H, 0:W]
        px = np.where((x // 64 + y // 24) % 2 == 0, 40 + 30 * ((x // 64 + y // 24) % 5), (x + 2 * y) // 3 % 256)[..., None] + np.arange(C) * 20
        px = np.broadcast_to(px, (B * H, W, C)).reshape(shape)
    else:  # "photo": a smooth field plus +-3 noise
        y, x = np.mgrid[0:B * H, 0:W]
        field = 128 + 60 * np.sin(x / 37.0) + 50 * np.cos(y / 23.0)
        px = (field[..., None] + np.arange(C) * 9 + rng.integers(-3, 4, (B * H, W, C))).reshape(shape)
    return np.clip(px, 0, 255).astype(np.uint8)


def fibonacci_row() -> np.ndarray:
    """one grey row whose byte values occur with Fibonacci counts (17710 in all): an unlimited Huffman code would reach 19 bits"""
    fib = [1, 1]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    row = np.repeat(np.arange(20) * 11 + 3, fib)
    return np.random.default_rng(4).permutation(row).astype(np.uint8).reshape(1, 1, -1, 1)


SHAPES = [(1, 1, 1), (1, 1, 7), (1, 5, 1), (1, 17, 33), (1, 33, 259), (2, 9, 20)]  # B, H, W
CASES = [(s, C, kind, "adaptive") for s in SHAPES for C in (1, 3) for kind in ("noise", "zeros", "single", "runs", "photo")]
CASES += [((1, 48, 1366), 3, kind, "adaptive") for kind in ("noise", "zeros", "photo")]      # a 16-row strip beyond one stored block
CASES += [((1, 2, 23300), 3, kind, "adaptive") for kind in ("noise", "photo")]               # a row beyond the strip target: strips in `work`
CASES += [((1, 17, 33), 3, "photo", f) for f in pr.FILTERS] + [((1, 33, 259), 3, "runs", "none"), ((2, 9, 20), 1, "runs", "none")]
CASES += [((1, 3, 400), 3, "runs", "none")]                                                  # a row that holds all six runs whole
CASES += [((1, 1, 17710), 1, "fibonacci", "none")]


@pytest.mark.parametrize("shape,C,kind,filt", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_file_decodes_to_the_pixels(ops, dev, shape, C, kind, filt):
    B, H, W = shape
    px = fibonacci_row() if kind == "fibonacci" else content(kind, B, H, W, C)
    px = px[..., 0] if C == 1 else px
    got = ops.png_encode(torch.from_numpy(px).to(dev), filter=filt)
    im = Image.open(io.BytesIO(got))
    im.load()                                                                                 # 1. every chunk CRC, the Adler-32
    assert im.mode == ("L" if C == 1 else "RGB") and im.size == (W, B * H)
    assert np.array_equal(np.asarray(im), px.reshape((B * H, W) + px.shape[3:]))              # 2. lossless
    assert zlib.decompress(pr.idat_payload(got)) == pr.filtered(px, filt).tobytes()           # 3. the filter choice and the tie rule
    assert len(got) <= pr.file_bound(B * H, W, C)                                             # 4. the definition's bound
    # 5. nothing behind the file is written; 6. a second run and a strided window give the same bytes
    nwork, cap = ops.png_workspace_bytes(B, H, W, C)
    work = torch.empty(nwork, dtype=torch.uint8, device=dev)
    wide = torch.full((B, H + 2, W * C + 5), 77, dtype=torch.uint8, device=dev)
    wide[:, :H, :W * C] = torch.from_numpy(px).to(dev).reshape(B, H, W * C)
    window = wide[:, :H, :W * C] if C == 1 else wide[:, :H, :W * C].unflatten(-1, (W, C))
    for cap_here in (cap, len(got)):
        buf = torch.full((cap_here + 64,), SENTINEL, dtype=torch.uint8, device=dev)
        n = ops.png_encode_into(window, work, buf[:cap_here], filt)
        host = buf.cpu().numpy()
        assert n == len(got) and bool((host[n:] == SENTINEL).all())
        ops.png_seal(host[:n])
        assert host[:n].tobytes() == got


# measured on the GPU (profiles/png.txt): photo 63871 / 63667 bytes = 1.0032, flat 10275 / 10071 bytes = 1.0203; the gates are those
# ratios plus one percentage point
@pytest.mark.parametrize("kind,gate", [("photo", 1.0132), ("flat", 1.0303)])
def test_size_against_zlib_rle(ops, dev, kind, gate):
    """96 x 512 x 3: the file against zlib level 6, Z_RLE, over the same filtered bytes strip by strip (optimal coding of the same tokens)."""
    px = content(kind, 1, 96, 512, 3)
    got = ops.png_encode(torch.from_numpy(px).to(dev))
    rows = pr.filtered(px)
    ref = 0
    for y0, y1 in pr.strips(96, 512, 3):
        z = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
        ref += len(z.compress(rows[y0:y1].tobytes()) + z.flush())
    print(f"png size {kind}: native {len(got)} bytes, zlib Z_RLE by strip {ref} bytes, ratio {len(got) / ref:.4f}")
    assert len(got) <= gate * ref


def test_too_small_out_is_refused_by_name(ops, dev):
    px = torch.from_numpy(content("noise", 1, 17, 33, 3)).to(dev)
    nwork, cap = ops.png_workspace_bytes(1, 17, 33, 3)
    work = torch.empty(nwork, dtype=torch.uint8, device=dev)
    n = len(ops.png_encode(px))
    buf = torch.full((n - 1 + 64,), SENTINEL, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="out_cap"):
        ops.png_encode_into(px, work, buf[:n - 1])
    assert bool((buf[n - 1:] == SENTINEL).all())
    with pytest.raises(RuntimeError, match="work holds"):
        ops.png_encode_into(px, work[:nwork - 256], buf)


# ---- the pipeline -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe(dev):
    from test_cfg_gpu import tiny_pipeline

    p = tiny_pipeline(dev)
    p.compile()
    return p


@pytest.mark.parametrize("num_images", [1, 2])
def test_pipeline_png(dev, pipe, num_images):
    from test_cfg_gpu import prompts

    pos, _ = prompts()
    kw = dict(width=64, height=96, num_steps=4, seed=7, silent=True, num_images=num_images)
    jpeg = pipe.generate(pos, output_type="jpeg", **kw).getvalue()
    px = np.asarray(pipe.generate(pos, output_type="uint8", **kw)).reshape(num_images * 96, 64, 3)
    native = pipe.generate(pos, output_type="png", **kw).getvalue()
    assert native == pipe.generate(pos, output_type="png", png_encoder="native", **kw).getvalue()
    pil = pipe.generate(pos, output_type="png", png_encoder="pil", **kw).getvalue()
    assert native != pil and pil == pipe._png(torch.from_numpy(px.reshape(num_images, 96, 64, 3))).getvalue()
    for data in (native, pil):
        assert data[:8] == b"\x89PNG\r\n\x1a\n" and np.array_equal(np.asarray(Image.open(io.BytesIO(data))), px)
    # a JPEG request is the request it was
    assert pipe.generate(pos, output_type="jpeg", **kw).getvalue() == jpeg == pipe._jpeg(torch.from_numpy(px.reshape(num_images, 96, 64, 3)), 99).getvalue()
    x = torch.rand(2, 3, 24, 40, generator=torch.Generator().manual_seed(1)).mul(2).sub(1).to(dev)
    for enc in ("native", "pil"):
        data = pipe.into_bytes(x, output_type="png", png_encoder=enc).getvalue()
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), pipe.to_uint8(x).numpy().reshape(48, 40, 3))
    with pytest.raises(ValueError, match="png_encoder='webp'"):
        pipe.generate(pos, output_type="png", png_encoder="webp", **kw)


def test_pipeline_png_tiled_flowedit_upscale(dev, pipe):
    """every request that returns pixels returns them as a PNG too: the file decodes to that request's uint8 array"""
    from fluxmi import synth
    from modules.upscaler import RRDBNet
    from test_cfg_gpu import prompts

    pos, neg = prompts()
    kw = dict(width=64, height=64, num_steps=4, seed=3, silent=True)
    photo = torch.randint(0, 256, (64, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    pipe.upscaler = RRDBNet(synth.make_rrdbnet_state_dict(1, 64, 32, 4, seed=21), device=dev)
    try:
        for extra in (dict(width=96, height=96, tile_size=64, tile_overlap=32), dict(init_image=photo, source_prompt=neg, num_steps=6),
                      dict(upscale=True)):
            torch.manual_seed(31)
            px = np.asarray(pipe.generate(pos, output_type="uint8", **dict(kw, **extra)))
            for enc in ("native", "pil"):
                torch.manual_seed(31)
                data = pipe.generate(pos, output_type="png", png_encoder=enc, **dict(kw, **extra)).getvalue()
                assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), px.reshape((-1,) + px.shape[2:]))
    finally:
        pipe.upscaler = None
