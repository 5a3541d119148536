"""fp64 reference of guidance shaping (include/fluxmi.h, fluxmi_guidance_combine), for tests/test_guidance_cpu.py and tests/test_guidance_gpu.py.

shape_vector: the rules written from their VECTOR definitions, per image, in float64 numpy -- the difference d, its norm clip, the projection
on c, the std ratio of diffusers' rescale_noise_cfg over all non-batch dimensions, CFG-Zero*'s optimised scale s* -- with no use of the moment
algebra.  coefficients: the closed forms of the header, from the nine sums.  The two must agree (test_guidance_cpu.py); the kernels are
compared with both.

params = (s, phi, eta, rho, mu, mode, zero_init, 0) as the kernel reads them: fp32 values (as_params rounds them), mode 0 = CFG, 1 = APG,
2 = CFG-Zero*.  `evaluation` = *step + *step_offset."""
import math

import numpy as np

MODES = {"cfg": 0, "apg": 1, "cfg_zero_star": 2}
SUMS = ("Sc", "Su", "Sr", "cc", "uu", "rr", "cu", "cr", "ur")


def as_params(s, mode="cfg", phi=0.0, eta=1.0, rho=0.0, mu=0.0, zero_init=0):
    """the 8 floats, rounded to fp32 like the device copy, as python floats"""
    m = MODES[mode] if isinstance(mode, str) else int(mode)
    return tuple(float(np.float32(v)) for v in (s, phi, eta, rho, mu, m, zero_init, 0.0))


def moments(c, u, r=None):
    """the nine sums of one image in float64 (r None: its sums are 0)"""
    c, u = np.asarray(c, np.float64).ravel(), np.asarray(u, np.float64).ravel()
    r = np.zeros_like(c) if r is None else np.asarray(r, np.float64).ravel()
    return np.array([c.sum(), u.sum(), r.sum(), c @ c, u @ u, r @ r, c @ u, c @ r, u @ r], np.float64)


def abs_moments(c, u, r=None):
    """sum |term| of each of the nine sums: the scale of the summation error bound"""
    c, u = np.abs(np.asarray(c, np.float64).ravel()), np.abs(np.asarray(u, np.float64).ravel())
    r = np.zeros_like(c) if r is None else np.abs(np.asarray(r, np.float64).ravel())
    return np.array([c.sum(), u.sum(), r.sum(), c @ c, u @ u, r @ r, c @ u, c @ r, u @ r], np.float64)


def shape_vector(c, u, r, params, evaluation=0):
    """-> (p, r_new, info): the shaped prediction of ONE image from the vector definitions; r None = no running difference (mu counts as 0);
    r_new = the advanced running difference (None when mu == 0); info: s_star / tau / f where the rule has them"""
    s, phi, eta, rho, mu, mode, zero_init = (float(v) for v in params[:7])
    c, u = np.asarray(c, np.float64), np.asarray(u, np.float64)
    if r is None:
        mu = 0.0
    rr = np.zeros_like(c) if r is None else np.asarray(r, np.float64)
    info = {}
    mode = int(mode)
    if mode == 0:
        p = u + s * (c - u)
    elif mode == 2:
        uu = float((u * u).sum())
        s_star = 1.0 if uu == 0.0 else float((c * u).sum()) / uu
        info["s_star"] = s_star
        p = s_star * u + s * (c - s_star * u)
    elif mode == 1:
        d = c - u + mu * rr  # the running difference after this evaluation (diffusers' MomentumBuffer.update)
        norm = math.sqrt(float((d * d).sum()))
        tau = min(1.0, rho / norm) if rho > 0.0 and norm > 0.0 else 1.0
        info["tau"] = tau
        d = d * tau
        cc = float((c * c).sum())
        par = (float((d * c).sum()) / cc) * c if cc != 0.0 else np.zeros_like(c)
        perp = d - par
        p = c + (s - 1.0) * (perp + eta * par)
    else:
        raise ValueError(f"mode {mode}")
    f = 1.0
    if phi > 0.0:
        # rescale_noise_cfg: std over every non-batch dimension; the N / (N - 1) of torch's unbiased std cancels in the ratio
        std_c, std_p = float(np.std(c)), float(np.std(p))
        if std_p > 0.0:
            f = phi * (std_c / std_p) + (1.0 - phi)
            p = phi * (p * (std_c / std_p)) + (1.0 - phi) * p
    info["f"] = f
    if evaluation < zero_init:
        p = np.zeros_like(c)
    r_new = (c - u) + mu * rr if mu != 0.0 else None
    return p, r_new, info


def coefficients(S, n, params, evaluation=0, has_r=True):
    """-> (alpha, beta, gamma, f) in float64 from the nine sums S of one image of n elements: the formulas of include/fluxmi.h"""
    Sc, Su, Sr, cc, uu, rr, cu, cr, ur = (float(v) for v in S)
    s, phi, eta, rho, mu, mode, zero_init = (float(v) for v in params[:7])
    if not has_r:
        mu = 0.0
    mode = int(mode)
    al, be, ga = s, 1.0 - s, 0.0
    if mode == 2:
        s_star = 1.0 if uu == 0.0 else cu / uu
        be = s_star * (1.0 - s)
    elif mode == 1:
        dd = cc + uu + mu * mu * rr - 2.0 * cu + 2.0 * mu * cr - 2.0 * mu * ur
        dc = cc - cu + mu * cr
        tau = min(1.0, rho / math.sqrt(dd)) if rho > 0.0 and dd > 0.0 else 1.0
        k = 0.0 if cc == 0.0 else tau * dc / cc
        al = 1.0 + (s - 1.0) * (tau + (eta - 1.0) * k)
        be = -(s - 1.0) * tau
        ga = (s - 1.0) * tau * mu
    f = 1.0
    if phi > 0.0:
        mean_p = (al * Sc + be * Su + ga * Sr) / n
        e_p2 = (al * al * cc + be * be * uu + ga * ga * rr + 2.0 * al * be * cu + 2.0 * al * ga * cr + 2.0 * be * ga * ur) / n
        var_p = e_p2 - mean_p * mean_p
        var_c = max(0.0, cc / n - (Sc / n) * (Sc / n))
        if var_p > 0.0:
            f = phi * math.sqrt(var_c / var_p) + (1.0 - phi)
        al, be, ga = al * f, be * f, ga * f
    if evaluation < zero_init:
        al = be = ga = 0.0
    return al, be, ga, f


def shape_coefficients(c, u, r, params, evaluation=0):
    """p = alpha c + beta u + gamma r in float64 with the coefficients of the exact float64 moments -> (p, (alpha, beta, gamma, f))"""
    c, u = np.asarray(c, np.float64), np.asarray(u, np.float64)
    co = coefficients(moments(c, u, r), c.size, params, evaluation, has_r=r is not None)
    p = co[0] * c + co[1] * u
    if r is not None:
        p = p + co[2] * np.asarray(r, np.float64)
    return p, co
