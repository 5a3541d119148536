"""Helpers of tests/test_solvers_cpu.py and tests/test_solvers_gpu.py: a torch interpreter of a fluxmi.solvers.SolverProgram.

Row j of a program updates x from the model's prediction v:

    g   = ga * x + gb * v
    acc = cx * x + cs * xs + c0 * g + c1 * hist[h1_slot] + c2 * hist[h2_slot]            left to right

A term whose coefficient is exactly 0 (as the arithmetic sees it) or whose slot is -1 is skipped and its buffer not read; the sum starts at
the first term present.  Then save_xs stores the PRE-update x to xs, w_slot >= 0 stores g to hist[w_slot], and x' = acc.

exact=True: float64 tensors, no rounding -- the mathematics of the program.
exact=False: the kernel's arithmetic (csrc/update_step.hip, solver_step_kernel) restated: x, v, xs bf16, hist fp32, the coefficients cast to
fp32; torch.mul and torch.add on fp32 tensors are separate operations, one rounding each (no fma); x1 = bf16(acc).  The guided chain and the
blend tail are inpaint_util.blend_step's expressions (bf16 tensors, python scalars)."""
import torch

import inpaint_util as iu


def f32(v):
    return torch.tensor(float(v), dtype=torch.float64).to(torch.float32)


def new_state(like, exact=False, fill=0.0):
    """(xs, hist) for a stream shaped like `like`: xs in its dtype, hist [2, ...] fp32 (exact: both float64)"""
    xs = torch.full_like(like, fill, dtype=torch.float64 if exact else torch.bfloat16)
    hist = torch.full((2,) + tuple(like.shape), fill, dtype=torch.float64 if exact else torch.float32, device=like.device)
    return xs, hist


def apply_row(x, v, row, ctl, xs, hist, exact=False, scale=None, blend=None):
    """One evaluation's update -> x'.  xs and hist are updated IN PLACE.  v = the prediction, or (c, u) with `scale` for the guided form.
    blend = (x0, noise, mask, t_next, thr or None): the masked-latent blend behind the update (exact=False only)."""
    if scale is not None:
        c, u = v
        v = u + scale * (c - u)
    if exact:
        X, V, k = x, v, float
    else:
        assert x.dtype == torch.bfloat16 and v.dtype == torch.bfloat16 and xs.dtype == torch.bfloat16 and hist.dtype == torch.float32
        X, V, k = x.float(), v.float(), f32
    cx, cs, c0, c1, c2, ga, gb = (k(c) for c in row[:7])
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
        terms.append(torch.mul(xs if exact else xs.float(), cs))
    if c0 != 0:
        terms.append(torch.mul(g, c0))
    if c1 != 0 and h1 >= 0:
        terms.append(torch.mul(hist[h1], c1))
    if c2 != 0 and h2 >= 0:
        terms.append(torch.mul(hist[h2], c2))
    acc = total(terms)
    x1 = acc if exact else acc.to(torch.bfloat16)
    if blend is not None:
        x0, noise, m, t_next, thr = blend
        x1 = iu.blend(x1, x0, noise, m, t_next, thr)
    if save:
        xs.copy_(x)
    if w >= 0:
        hist[w].copy_(g)
    return x1


def run_program(prog, x, field, exact=False, **kw):
    """the whole program on x with v = field(x, t, j) at evaluation j -> the final x"""
    xs, hist = new_state(x, exact)
    for j, (row, ctl) in enumerate(zip(prog.coef, prog.ctl)):
        x = apply_row(x, field(x, prog.times[j], j), row, ctl, xs, hist, exact=exact, **kw)
    return x
