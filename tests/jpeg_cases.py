"""The inputs of the JPEG tests: the case list tests/test_jpeg_gpu.py runs on the device and tests/test_jpeg_cpu.py checks for coverage (every
path of the entropy coder must occur in it), and the images' makers.  A case is (family, B, H, W, quality, subsampling, restart); restart
None = the encoder's default, 0 = no restart markers."""
import functools

import numpy as np

import jpeg_ref

DEFAULT_RESTART = {"4:2:0": 4, "4:4:4": 8}  # fluxmi.ops.JPEG_DEFAULT_RESTART (test_jpeg_cpu.py checks they agree)
SIZES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 33), (64, 48), (250, 130)]  # W x H
FAMILIES = ["noise", "ramp", "impulse", "const0", "const255", "checker8", "checker4", "photo"]


def make_image(family: str, B: int, H: int, W: int, seed: int = 0) -> np.ndarray:
    """uint8 [B, H, W, 3]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:B * H, 0:W]
    if family == "noise":
        im = rng.integers(0, 256, (B * H, W, 3))
    elif family == "ramp":      # smooth, a different slope per channel
        im = np.stack([(xx * 255) // max(W - 1, 1), (yy * 255) // max(B * H - 1, 1), ((xx + yy) * 255) // max(W + B * H - 2, 1)], -1)
    elif family == "impulse":   # one bright pixel per 8 x 8 block, elsewhere dark grey
        im = np.full((B * H, W, 3), 16)
        im[(yy % 8 == 3) & (xx % 8 == 5)] = (255, 240, 200)
    elif family == "const0":
        im = np.zeros((B * H, W, 3))
    elif family == "const255":
        im = np.full((B * H, W, 3), 255)
    elif family == "checker8":  # 8-pixel squares of 0 / 255 on the block grid: every block constant, full-scale DC steps block to block
        im = np.repeat((((yy // 8) + (xx // 8)) % 2 * 255)[..., None], 3, -1)
    elif family == "checker4":  # the same squares 4 pixels to the right: every block a full-scale step whose sign flips block to block
        im = np.repeat((((yy // 8) + ((xx + 4) // 8)) % 2 * 255)[..., None], 3, -1)
    elif family == "photo":     # smooth structure + sensor-like noise
        base = np.stack([128 + 100 * np.sin(xx / 9.0 + yy / 17.0), 128 + 90 * np.cos(xx / 13.0 - yy / 7.0), 60 + yy * 150.0 / max(B * H, 1)], -1)
        im = np.clip(base + rng.normal(0, 6, base.shape), 0, 255)
    else:
        raise KeyError(family)
    return np.ascontiguousarray(im.astype(np.uint8).reshape(B, H, W, 3))


def _cases():
    out = []
    # every size x both subsamplings, the other axes rotating so that each value of each occurs
    qs, rs, fams = [99, 1, 50, 90, 100], [None, 0, 1, 3, 60000], ["noise", "ramp", "impulse", "photo"]
    i = 0
    for (W, H) in SIZES:
        for ss in ("4:2:0", "4:4:4"):
            out.append((fams[i % 4], 3 if i % 3 == 1 else 1, H, W, qs[i % 5], ss, rs[(i // 2 + i) % 5]))
            i += 1
    out += [
        # the paths of the entropy coder (test_jpeg_cpu.py::test_case_list_covers_every_path says which case is for what)
        ("checker8", 1, 48, 64, 100, "4:4:4", 1),        # DC differences of category 11; RST0..7 and the wrap (48 MCUs)
        ("checker8", 1, 48, 64, 100, "4:2:0", 1),
        ("checker4", 1, 48, 64, 100, "4:4:4", None),     # AC levels of category 10
        ("checker4", 3, 33, 17, 100, "4:2:0", 3),
        ("const0", 1, 33, 17, 99, "4:2:0", None),        # EOB-only blocks
        ("const255", 3, 7, 5, 99, "4:4:4", 0),
        ("const255", 1, 130, 250, 50, "4:2:0", 1),
        ("noise", 1, 48, 64, 100, "4:4:4", 0),           # blocks without EOB, stuffed 0xFF, one long interval
        ("noise", 1, 48, 64, 100, "4:2:0", None),
        ("noise", 3, 7, 5, 100, "4:2:0", 1),             # stacking crosses MCU rows (7 % 16 != 0)
        ("noise", 3, 33, 17, 90, "4:4:4", 3),
        ("noise", 1, 130, 250, 1, "4:2:0", None),        # ZRLs
        ("noise", 1, 130, 250, 50, "4:4:4", 3),
        ("photo", 1, 130, 250, 99, "4:2:0", None),
        ("photo", 3, 48, 64, 90, "4:2:0", 0),
        ("ramp", 1, 130, 250, 90, "4:4:4", None),
        ("ramp", 1, 24, 40, 99, "4:2:0", 1),             # an even height that is no multiple of 16: the last chroma row repeats
        ("impulse", 1, 48, 64, 99, "4:2:0", 60000),      # an interval larger than the image
        ("impulse", 3, 16, 16, 50, "4:4:4", 1),
    ]
    return out


CASES = _cases()
# thousands of intervals: the offsets' prefix sum walks several intervals per thread
BIG_CASES = [("noise", 1, 384, 512, 99, "4:2:0", None), ("noise", 1, 384, 512, 99, "4:4:4", 1)]


def case_id(c) -> str:
    fam, B, H, W, q, ss, R = c
    return f"{fam}-{B}x{H}x{W}-q{q}-{ss.replace(':', '')}-R{'def' if R is None else R}"


def restart_of(c) -> int:
    return DEFAULT_RESTART[c[5]] if c[6] is None else c[6]


@functools.lru_cache(maxsize=None)
def image_of(c) -> np.ndarray:
    im = make_image(c[0], c[1], c[2], c[3], seed=len(case_id(c)) + c[4])
    im.setflags(write=False)
    return im


@functools.lru_cache(maxsize=None)
def reference_of(c):
    """(bytes, stats) of the reference encoder on the case: computed once, shared by the tests"""
    stats = jpeg_ref.new_stats()
    return jpeg_ref.jpeg_ref(image_of(c), c[4], c[5], restart_of(c), stats=stats), stats
