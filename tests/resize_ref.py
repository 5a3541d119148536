"""Pillow's 8-bit resampler (ImagingResample) restated: the definition behind fluxmi_resample_coeffs / fluxmi_resample_u8 (include/fluxmi.h).
Coefficients in double with libm's sin / cos (math, not numpy: another sin may differ in the last bit and move a coefficient across its
rounding step), rounded to 22-bit integers; each pass is integer arithmetic with a uint8 result, horizontal first."""
import math

import numpy as np

PRECISION_BITS = 22


def _sinc(x):
    return 1.0 if x == 0.0 else math.sin(x * math.pi) / (x * math.pi)


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    return 1.0 - abs(x) if abs(x) < 1.0 else 0.0


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (float(np.float32(0.54)) + float(np.float32(0.46)) * math.cos(x))  # Pillow writes 0.54f and 0.46f


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


FILTERS = {"box": (_box, 0.5), "bilinear": (_bilinear, 1.0), "hamming": (_hamming, 1.0), "bicubic": (_bicubic, 2.0), "lanczos": (_lanczos, 3.0)}


def coeffs(n_in: int, n_out: int, filter: str):
    """one axis -> (bounds int32 [n_out, 2] of (xmin, n), kk int32 [n_out, ksize], zero-padded)"""
    f, s = FILTERS[filter]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = s * fs
    ksize = 2 * int(math.ceil(support)) + 1
    ss = 1.0 / fs
    bounds = np.zeros((n_out, 2), np.int32)
    kk = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = xmin, n
        kk[xx, :n] = [int(v * (1 << PRECISION_BITS) + (-0.5 if v < 0 else 0.5)) for v in w]
    return bounds, kk


def one_pass(img: np.ndarray, axis: int, n_out: int, filter: str) -> np.ndarray:
    """img uint8 [H, W, C] resampled along `axis` (0 = rows, 1 = columns) to n_out samples"""
    bounds, kk = coeffs(img.shape[axis], n_out, filter)
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    out = np.empty((n_out,) + src.shape[1:], np.uint8)
    for xx, (xmin, n) in enumerate(bounds):
        acc = np.tensordot(kk[xx, :n], src[xmin:xmin + n], axes=(0, 0)).astype(np.int32) + (1 << (PRECISION_BITS - 1))
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img: np.ndarray, size, filter: str = "lanczos") -> np.ndarray:
    """img uint8 [H, W] or [H, W, C] -> size = (width, height), as PIL.Image.resize(size, filter) of an "L" / "RGB" image"""
    x = img[:, :, None] if img.ndim == 2 else img
    w, h = size
    if w != x.shape[1]:
        x = one_pass(x, 1, w, filter)
    if h != x.shape[0]:
        x = one_pass(x, 0, h, filter)
    return x[:, :, 0] if img.ndim == 2 else x
