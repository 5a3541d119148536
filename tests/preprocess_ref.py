"""numpy references of the control-map preprocessors (csrc/preprocess.hip): the Canny definition of include/fluxmi.h in int64, hysteresis by
connected components, PIL's luma formula, the Gaussian blur in fp64; and the input families the CPU and GPU tests share."""
import math

import numpy as np
from scipy import ndimage

TILE = 32  # FLUXMI_CANNY_TILE (both Canny kernels)


# ---- Canny -----------------------------------------------------------------------------------------------------------------------------
def sobel(rgb: np.ndarray, l2: bool = False):
    """rgb uint8 [H, W, 3] -> (dx, dy, m) int64 [H, W] of the channel with the largest magnitude (lowest index wins ties)"""
    p = np.pad(rgb.astype(np.int64), ((1, 1), (1, 1), (0, 0)), mode="edge")
    dx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    dy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    m = dx * dx + dy * dy if l2 else np.abs(dx) + np.abs(dy)
    bdx, bdy, bm = dx[..., 0].copy(), dy[..., 0].copy(), m[..., 0].copy()
    for c in (1, 2):
        take = m[..., c] > bm
        bdx[take], bdy[take], bm[take] = dx[..., c][take], dy[..., c][take], m[..., c][take]
    return bdx, bdy, bm


def canny_classify(rgb: np.ndarray, low: int, high: int, l2: bool = False) -> np.ndarray:
    """rgb uint8 [H, W, 3] (or a batch [B, H, W, 3]) -> state uint8: 0, 1 (weak) or 2 (strong)"""
    if rgb.ndim == 4:
        return np.stack([canny_classify(x, low, high, l2) for x in rgb])
    lo, hi = min(low, high), max(low, high)
    if l2:
        lo, hi = lo * lo, hi * hi
    dx, dy, m = sobel(rgb, l2)
    H, W = m.shape
    mp = np.pad(m, 1)  # magnitudes outside the image count as 0
    nb = lambda oy, ox: mp[1 + oy:1 + oy + H, 1 + ox:1 + ox + W]
    x, y = np.abs(dx), np.abs(dy) << 15
    t22 = x * 13573
    t67 = t22 + (x << 16)
    horiz = y < t22
    vert = ~horiz & (y > t67)
    keep_h = (m > nb(0, -1)) & (m >= nb(0, 1))
    keep_v = (m > nb(-1, 0)) & (m >= nb(1, 0))
    opposite = (dx < 0) != (dy < 0)  # s = -1: up-right and down-left
    keep_d = np.where(opposite, (m > nb(-1, 1)) & (m > nb(1, -1)), (m > nb(-1, -1)) & (m > nb(1, 1)))
    keep = np.where(horiz, keep_h, np.where(vert, keep_v, keep_d)) & (m > lo)
    return np.where(keep, np.where(m > hi, 2, 1), 0).astype(np.uint8)


def hysteresis(state: np.ndarray) -> np.ndarray:
    """state uint8 [H, W] (or [B, H, W]) of 0 / 1 / 2 -> edges uint8: 255 on every 8-connected component of non-zero pixels that holds a 2"""
    if state.ndim == 3:
        return np.stack([hysteresis(s) for s in state])
    lab, _ = ndimage.label(state > 0, structure=np.ones((3, 3), dtype=bool))
    strong = np.unique(lab[state == 2])
    return (np.isin(lab, strong) & (lab > 0)).astype(np.uint8) * 255


def canny(rgb: np.ndarray, low: int, high: int, l2: bool = False) -> np.ndarray:
    return hysteresis(canny_classify(rgb, low, high, l2))


# ---- luma, blur ------------------------------------------------------------------------------------------------------------------------
def gray(rgb: np.ndarray) -> np.ndarray:
    v = rgb.astype(np.int64)
    return ((19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 32768) >> 16).astype(np.uint8)


def blur_taps(sigma: float) -> np.ndarray:
    r = math.ceil(3.0 * float(np.float32(sigma)))
    i = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-i * i / (2.0 * float(np.float32(sigma)) ** 2))
    return w / w.sum()


def blur_f64(img: np.ndarray, sigma: float) -> np.ndarray:
    """img uint8 [..., H, W, C] -> fp64, the separable Gaussian with a replicated border, unrounded"""
    w = blur_taps(sigma)
    r = len(w) // 2
    x = img.astype(np.float64)
    H, W = x.shape[-3], x.shape[-2]
    pad = [(0, 0)] * x.ndim
    pad[-2] = (r, r)
    xp = np.pad(x, pad, mode="edge")
    t = sum(w[i] * xp[..., i:i + W, :] for i in range(2 * r + 1))
    pad = [(0, 0)] * x.ndim
    pad[-3] = (r, r)
    tp = np.pad(t, pad, mode="edge")
    return sum(w[i] * tp[..., i:i + H, :, :] for i in range(2 * r + 1))


def blur_excused(ref: np.ndarray) -> np.ndarray:
    """pixels whose fp64 value lies within 2^-10 of a half-integer: the fp32 kernel may round them either way"""
    return np.abs(ref - np.floor(ref) - 0.5) <= 2.0 ** -10


# ---- input families --------------------------------------------------------------------------------------------------------------------
FAMILIES = ("noise", "smooth", "constant", "checker", "channels", "equal")


def family(name: str, H: int, W: int, seed: int = 0) -> np.ndarray:
    """uint8 [H, W, 3]"""
    rng = np.random.default_rng([seed, H, W, FAMILIES.index(name)])
    yy, xx = np.mgrid[0:H, 0:W]
    if name == "noise":  # dense edges
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if name == "smooth":  # ramps plus a few discs and bars: long thin edges, weak and strong
        img = np.stack([xx * 255.0 / max(W - 1, 1), yy * 255.0 / max(H - 1, 1), (xx + yy) * 255.0 / max(H + W - 2, 1)], -1) * 0.5
        for _ in range(4):
            cy, cx, rad = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(2, max(3.0, min(H, W) / 3))
            img[(yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad] += rng.uniform(-120, 120, 3)
        for _ in range(3):
            a, b = sorted(rng.integers(0, W + 1, 2))
            img[:, a:min(b, a + 5)] += rng.uniform(-60, 60, 3)
            a, b = sorted(rng.integers(0, H + 1, 2))
            img[a:min(b, a + 3)] += rng.uniform(-25, 25, 3)
        return np.clip(np.rint(img), 0, 255).astype(np.uint8)
    if name == "constant":
        return np.full((H, W, 3), 137, dtype=np.uint8)
    if name == "checker":  # a 1-pixel checkerboard
        return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
    if name == "channels":  # the strongest edge of each channel lies somewhere else
        img = rng.integers(0, 12, (H, W, 3)).astype(np.int64)
        img[:, W // 4:, 0] += 200
        img[H // 2:, :, 1] += 170
        img[(xx + yy) > (H + W) // 2, 2] += 230
        img[:, (3 * W) // 4:, 1] += 60
        return np.clip(img, 0, 255).astype(np.uint8)
    if name == "equal":  # equal channels: every magnitude is a three-way tie
        g = family("smooth", H, W, seed + 1)[..., 0].astype(np.int64) + rng.integers(0, 40, (H, W))
        return np.repeat(np.clip(g, 0, 255).astype(np.uint8)[..., None], 3, -1)
    raise KeyError(name)


# ---- synthetic state maps for the hysteresis kernel ------------------------------------------------------------------------------------
def serpentine(H: int, W: int, pitch: int = 4, gap=None) -> np.ndarray:
    """A 1-pixel-wide path of weak pixels: every `pitch`-th row in full, joined alternately at the right and the left edge, with ONE strong
    pixel at its start (0, 0).  `gap` = (row index of the path, column): that pixel is removed, which cuts the path in two."""
    s = np.zeros((H, W), dtype=np.uint8)
    rows = list(range(0, H, pitch))
    for k, y in enumerate(rows):
        s[y, :] = 1
        if k + 1 < len(rows):
            s[y:rows[k + 1], W - 1 if k % 2 == 0 else 0] = 1
    s[0, 0] = 2
    if gap is not None:
        assert 2 <= gap[1] < W - 2  # away from the joins, so the cut is a cut under 8-connectivity
        s[rows[gap[0]], gap[1]] = 0
    return s


# ---- the blur cases of the GPU test: (sigma, C, H, W, seed).  tests/test_preprocess_cpu.py checks that the fp64 reference alone puts under
# 1 % of each case's values within 2^-10 of a half-integer (the pixels the fp32 kernel may round either way)
BLUR_SIZES = ((1, 1), (1, 7), (2, 3), (31, 65), (64, 64), (33, 63), (67, 193), (70, 300))
BLUR_CASES = tuple((sigma, C, H, W, 11) for sigma in (0.5, 2.0, 8.0) for C in (1, 3) for (H, W) in BLUR_SIZES)


def blur_input(C: int, H: int, W: int, seed: int, B: int = 1) -> np.ndarray:
    """uint8 [B, H, W, C]: noise on top of a ramp, so that blurred values spread over the whole range"""
    rng = np.random.default_rng([seed, C, H, W])
    yy, xx = np.mgrid[0:H, 0:W]
    base = ((xx * 3 + yy * 5) % 256)[None, ..., None]
    return ((base + rng.integers(0, 200, (B, H, W, C))) % 256).astype(np.uint8)
