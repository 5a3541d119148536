"""References of the latent preview (include/fluxmi.h, fluxmi_latent_preview), for tests/test_preview_cpu.py and tests/test_preview_gpu.py.

  reference_fp64   the definition in float64 on the kernel's OPERANDS (bf16 x / pred, fp32 t, s and factors, all exactly representable):
                   the pre-rounding level y = (0.5 rgb + 0.5) * 255, the uint8 image, and the per-pixel band half-width
                       delta = 20 * 2^-24 * 127.5 * (|bias| + sum_c |M[c]| |x0_c|)
                   -- the forward-error bound of the 17-term fma chain (gamma_17), one unit for the x0 fma and two for the final fma and
                   product, on the scale of the levels (rgb -> y multiplies by 127.5).
  emulate_fp32     the kernel's operation order in NumPy float32; an fma is the exact float64 product plus the addend, rounded to fp32
                   (24 + 24-bit products are exact in float64; the double rounding this leaves moves a result by at most one fp32 ulp in
                   rare cases, which the band covers).
  check_band       the comparison rule: equal outside the band, at most one level apart inside it.
All take NumPy arrays: x [B (2B guided), img_rows, c_in], pred [B (2B guided), pred_rows, 64] as float32 holding bf16 values."""
import numpy as np

U = 2.0 ** -24


def _operands(x, pred, grid, guided):
    h, w = grid
    B = x.shape[0] // 2 if guided else x.shape[0]
    n = h * w
    assert pred.shape[1] == n and pred.shape[2] == 64 and x.shape[1] >= n and x.shape[2] >= 64
    # [B, n, 16 channels, 4 sub-pixels]: packed column c * 4 + sub
    xv = x[:B, :n, :64].reshape(B, n, 16, 4)
    c = pred[:B].reshape(B, n, 16, 4)
    u = pred[B:2 * B].reshape(B, n, 16, 4) if guided else None
    return B, xv, c, u


def _to_image(a, B, h, w):
    """[B, n, 4 (py * 2 + px), 3] -> [B, 2 h, 2 w, 3]"""
    return a.reshape(B, h, w, 2, 2, 3).transpose(0, 1, 3, 2, 4, 5).reshape(B, 2 * h, 2 * w, 3)


def quantise(y):
    """rint (half to even), clamp to 0..255, NaN -> 0"""
    with np.errstate(invalid="ignore"):
        q = np.rint(y)
        q = np.where(q > 0, np.where(q < 255, q, 255), 0)
    return q.astype(np.uint8)


def reference_fp64(x, pred, t, proj, grid, scale=None):
    """-> (uint8 [B, 2h, 2w, 3], y float64 pre-rounding levels, delta float64 band half-widths), each [B, 2h, 2w, 3]"""
    guided = scale is not None
    B, xv, c, u = _operands(np.asarray(x, np.float64), np.asarray(pred, np.float64), grid, guided)
    t = float(np.float32(t))
    proj = np.asarray(proj, np.float32).astype(np.float64)
    M, bias = proj[:48].reshape(16, 3), proj[48:]
    with np.errstate(invalid="ignore", over="ignore"):
        v = u + float(np.float32(scale)) * (c - u) if guided else c
        x0 = xv - t * v                                            # [B, n, 16, 4]
        rgb = bias + np.einsum("bncs,ck->bnsk", x0, M)             # [B, n, 4, 3]
        mag = np.abs(bias) + np.einsum("bncs,ck->bnsk", np.abs(x0), np.abs(M))
        y = (0.5 * rgb + 0.5) * 255.0
    h, w = grid
    y, delta = _to_image(y, B, h, w), _to_image(20 * U * 127.5 * mag, B, h, w)
    return quantise(y), y, delta


def emulate_fp32(x, pred, t, proj, grid, scale=None):
    """the kernel's fp32 operation order -> uint8 [B, 2h, 2w, 3]"""
    guided = scale is not None
    B, xv, c, u = _operands(np.asarray(x, np.float32), np.asarray(pred, np.float32), grid, guided)
    f32, f64 = np.float32, np.float64
    fma = lambda a, b, d: (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(d, f64)).astype(f32)
    t, proj = f32(t), np.asarray(proj, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = fma(f32(scale), (c - u).astype(f32), u) if guided else c
        x0 = fma(-t, v, xv)
        acc = np.broadcast_to(proj[48:], x0.shape[:2] + (4, 3)).astype(f32)
        for ch in range(16):
            acc = fma(proj[3 * ch:3 * ch + 3][None, None, None, :], x0[:, :, ch, :, None], acc)
        y = (fma(f32(0.5), acc, f32(0.5)) * f32(255.0)).astype(f32)
    h, w = grid
    return quantise(_to_image(y, B, h, w))


def in_band(y, delta):
    """pixels whose fp64 level lies within delta of a half-integer (where rint may legitimately go either way), NaN levels excluded"""
    with np.errstate(invalid="ignore"):
        frac = np.abs(y - np.floor(y) - 0.5)
        return (frac <= delta) & (y > -1.0) & (y < 256.0)


def check_band(got, want, y, delta, what=""):
    """got == want outside the band; inside it at most one level apart.  Returns the share of pixels inside the band."""
    got, want = np.asarray(got).astype(np.int32), np.asarray(want).astype(np.int32)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    band = in_band(y, delta)
    diff = np.abs(got - want)
    bad = (diff != 0) & ~band
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ outside the band (max |d| {int(diff[bad].max())}), first at {np.argwhere(bad)[0]}"
    assert diff.max(initial=0) <= 1, f"{what}: a pixel inside the band is {int(diff.max())} levels off"
    return float(band.mean())


def bf16_round(a):
    """float32 array -> the nearest bf16 values (RNE), as float32"""
    a = np.ascontiguousarray(a, np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def draws(B, grid, seed, guided=False, img_rows=None, c_in=64, amp=1.0):
    """seeded bf16-valued operands: x [B (2B), img_rows, c_in], pred [B (2B), h w, 64], a projection with O(1) rows, t and s"""
    rng = np.random.default_rng(seed)
    n = grid[0] * grid[1]
    Bx = 2 * B if guided else B
    x = bf16_round(amp * rng.standard_normal((Bx, img_rows or n, c_in)).astype(np.float32))
    pred = bf16_round(amp * rng.standard_normal((Bx, n, 64)).astype(np.float32))
    proj = np.concatenate([0.15 * rng.standard_normal(48), 0.1 * rng.standard_normal(3)]).astype(np.float32)
    return x, pred, proj, np.float32(0.6180339887), np.float32(3.5)
