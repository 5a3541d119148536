"""Helpers of tests/test_stochastic_cpu.py and tests/test_stochastic_gpu.py: a numpy reference of the kernel's counter-based generator and the
interpreter of tests/solver_util.py extended by the noise term.

Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) with the published constants.  Element e of
image b's dense block belongs to block q = e // 4: counter (q, eval, ids[b][2], ids[b][3]), key (ids[b][0], ids[b][1]) -> words w0..w3 ->

    u = ((w_even >> 9) + 0.5) * 2^-23 in (0, 1),   t = (w_odd >> 8) * 2^-24 in [0, 1)         (both exact in fp32)
    r = sqrt(-2 log u),   z = r cos(2 pi t), r sin(2 pi t)   from (w0, w1), then from (w2, w3)

apply_row restates solver_step_kernel's NOISE form (csrc/update_step.hip): fp32 products and sums one by one, left to right, the noise term
cn * z last, one bf16 store, then the blend."""
import numpy as np
import torch

import inpaint_util as iu
import solver_util as su

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: 4 uint32 arrays (or ints) broadcastable against each other, key: 2 -> 4 uint32 arrays"""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    k = [int(v) & MASK for v in key]
    c = list(np.broadcast_arrays(*c))
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # < 2^64: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k[0]), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k[1]), p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return [v.astype(np.uint32) for v in c]


def words(ids, n, ev):
    """the uint32 words of one image: ids = (key_lo, key_hi, c2, c3), n elements (n % 4 == 0), evaluation index ev -> uint32 [n]"""
    assert n % 4 == 0
    q = np.arange(n // 4, dtype=np.uint64)
    w = philox4x32_10((q, int(ev), int(ids[2]), int(ids[3])), (ids[0], ids[1]))
    return np.stack(w, axis=1).reshape(n)


def normals64(w):
    """float64 Box-Muller of the words uint32 [n] in the kernel's pairing -> float64 [n]"""
    w = np.asarray(w, dtype=np.uint32).reshape(-1, 2).astype(np.uint64)
    u = ((w[:, 0] >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    t = (w[:, 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u))
    return np.stack((r * np.cos(2.0 * np.pi * t), r * np.sin(2.0 * np.pi * t)), axis=1).reshape(-1)


def ids_of(seed, k, c3=0):
    """the pipeline's ids of image k of a request with noise seed `seed`"""
    return (seed & MASK, (seed >> 32) & MASK, k, c3)


def apply_row(x, v, row, ctl, xs, hist, z=None, scale=None, blend=None):
    """One evaluation's update in the kernel's arithmetic -> x' (bf16).  xs / hist are updated IN PLACE.  z: fp32 normals shaped like x,
    read only when the row's cn (column 7, as fp32) is not 0.  v, scale, blend as solver_util.apply_row."""
    if scale is not None:
        c, u = v
        v = u + scale * (c - u)
    assert x.dtype == torch.bfloat16 and v.dtype == torch.bfloat16 and xs.dtype == torch.bfloat16 and hist.dtype == torch.float32
    X, V = x.float(), v.float()
    cx, cs, c0, c1, c2, ga, gb, cn = (su.f32(c) for c in row)
    save, w, h1, h2 = (int(c) for c in ctl)

    def total(terms):
        acc = None
        for t in terms:
            acc = t if acc is None else torch.add(acc, t)
        return torch.zeros_like(X) if acc is None else acc

    g = None
    if c0 != 0 or w >= 0:
        g = total(([torch.mul(X, ga)] if ga != 0 else []) + ([torch.mul(V, gb)] if gb != 0 else []))
    terms = []
    if cx != 0:
        terms.append(torch.mul(X, cx))
    if cs != 0:
        terms.append(torch.mul(xs.float(), cs))
    if c0 != 0:
        terms.append(torch.mul(g, c0))
    if c1 != 0 and h1 >= 0:
        terms.append(torch.mul(hist[h1], c1))
    if c2 != 0 and h2 >= 0:
        terms.append(torch.mul(hist[h2], c2))
    if cn != 0:
        assert z is not None and z.dtype == torch.float32 and z.shape == x.shape
        terms.append(torch.mul(z, cn))
    x1 = total(terms).to(torch.bfloat16)
    if blend is not None:
        x0, noise, m, t_next, thr = blend
        x1 = iu.blend(x1, x0, noise, m, t_next, thr)
    if save:
        xs.copy_(x)
    if w >= 0:
        hist[w].copy_(g)
    return x1
