"""Guidance shaping, host side: the fp64 reference's two forms agree (tests/guidance_ref.py: the vector definitions against the closed-form
coefficients of include/fluxmi.h), the identities and degenerate fallbacks of the rules, and the refusals of Flux.denoise's argument check."""
import math

import numpy as np
import pytest

import guidance_ref as gr

N = 4096
CASES = {
    "cfg": dict(s=3.5),
    "cfg_rescale": dict(s=5.0, phi=0.7),
    "apg": dict(s=4.0, mode="apg", eta=0.25),
    "apg_clip": dict(s=4.0, mode="apg", eta=0.0, rho=7.5),
    "apg_momentum": dict(s=6.0, mode="apg", eta=0.5, rho=20.0, mu=-0.5),
    "apg_momentum_rescale": dict(s=6.0, mode="apg", eta=0.5, rho=5.0, mu=-0.75, phi=0.4),
    "zero_star": dict(s=3.0, mode="cfg_zero_star"),
    "zero_star_rescale": dict(s=7.0, mode="cfg_zero_star", phi=1.0),
}


def draws(seed, n=N):
    g = np.random.default_rng(seed)
    c = 0.3 + g.standard_normal(n)
    u = 0.6 * c + 0.5 * g.standard_normal(n)
    r = 0.8 * g.standard_normal(n)
    return c, u, r


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("with_r", [False, True], ids=["no_r", "r"])
def test_vector_and_coefficient_forms_agree(name, with_r):
    params = gr.as_params(**CASES[name])
    for seed in range(3):
        c, u, r = draws(seed)
        r = r if with_r else None
        p_vec, r_new, info = gr.shape_vector(c, u, r, params)
        p_co, co = gr.shape_coefficients(c, u, r, params)
        assert rel_l2(p_co, p_vec) <= 1e-12, f"{name} seed {seed}: {rel_l2(p_co, p_vec):.3e}"
        assert abs(co[3] - info["f"]) <= 1e-12 * abs(info["f"])
        mu = params[4] if with_r else 0.0
        if mu != 0.0:
            assert np.array_equal(r_new, (c - u) + mu * r)
        else:
            assert r_new is None
        if "tau" in info and name in ("apg_clip", "apg_momentum_rescale"):
            assert info["tau"] < 1.0, "the clip of this case is meant to bite"


def test_identities():
    c, u, r = draws(11)
    cfg = u + 3.5 * (c - u)
    # APG at eta = 1, rho = 0, mu = 0 is CFG
    p, _, _ = gr.shape_vector(c, u, r, gr.as_params(3.5, "apg", eta=1.0))
    assert rel_l2(p, cfg) <= 1e-12
    al, be, ga, f = gr.coefficients(gr.moments(c, u, r), N, gr.as_params(3.5, "apg"))
    assert (abs(al - 3.5) <= 1e-12 and abs(be + 2.5) <= 1e-12 and ga == 0.0 and f == 1.0)
    # phi = 0 is the identity, exactly
    for mode in gr.MODES:
        assert gr.coefficients(gr.moments(c, u, r), N, gr.as_params(3.5, mode, phi=0.0))[3] == 1.0
    assert np.array_equal(gr.shape_vector(c, u, None, gr.as_params(3.5))[0], cfg)
    # phi = 1: std(p) == std(c)
    for mode in gr.MODES:
        for form in (lambda pr: gr.shape_vector(c, u, r, pr)[0], lambda pr: gr.shape_coefficients(c, u, r, pr)[0]):
            p = form(gr.as_params(6.0, mode, phi=1.0, mu=-0.5 if mode == "apg" else 0.0))
            assert abs(np.std(p) / np.std(c) - 1.0) <= 1e-12, mode
    # CFG-Zero* with u = lambda c: s* = 1 / lambda, and the guided prediction is c whatever s is
    for lam in (0.5, -2.0, 3.0):
        p, _, info = gr.shape_vector(c, lam * c, None, gr.as_params(4.0, "cfg_zero_star"))
        assert abs(info["s_star"] - 1.0 / lam) <= 1e-12 and rel_l2(p, c) <= 1e-12
        al, be, _, _ = gr.coefficients(gr.moments(c, lam * c), N, gr.as_params(4.0, "cfg_zero_star"))
        assert abs(be - (1.0 / lam) * (1.0 - 4.0)) <= 1e-12 and al == 4.0
    # zero-init: 0 below zero_init, untouched at it; r still advances
    pz = gr.as_params(4.0, "apg", mu=-0.5, zero_init=2)
    for ev, zero in ((0, True), (1, True), (2, False), (5, False)):
        p, r_new, _ = gr.shape_vector(c, u, r, pz, evaluation=ev)
        co = gr.coefficients(gr.moments(c, u, r), N, pz, evaluation=ev)
        assert (not p.any()) == zero and (co[:3] == (0.0, 0.0, 0.0)) == zero
        assert np.array_equal(r_new, (c - u) - 0.5 * r)


def test_degenerate_sums_take_the_stated_fallbacks():
    c, u, r = draws(5)
    z = np.zeros(N)
    finite = lambda t: all(math.isfinite(v) for v in t)
    # uu == 0: s* = 1
    co = gr.coefficients(gr.moments(c, z), N, gr.as_params(3.0, "cfg_zero_star"))
    assert co == (3.0, -2.0, 0.0, 1.0)
    p, _, info = gr.shape_vector(c, z, None, gr.as_params(3.0, "cfg_zero_star"))
    assert info["s_star"] == 1.0 and np.array_equal(p, 3.0 * c)
    # cc == 0: k = 0 (no projection); dd > 0
    co = gr.coefficients(gr.moments(z, u), N, gr.as_params(3.0, "apg", eta=0.0, rho=1.0))
    assert finite(co) and co[2] == 0.0
    p, _, _ = gr.shape_vector(z, u, None, gr.as_params(3.0, "apg", eta=0.0, rho=1.0))
    assert np.isfinite(p).all() and rel_l2(co[0] * z + co[1] * u, p) <= 1e-12
    # dd == 0 (c == u, mu == 0): tau = 1, p = c
    co = gr.coefficients(gr.moments(c, c), N, gr.as_params(3.0, "apg", eta=0.3, rho=1.0))
    assert finite(co) and abs(co[0] + co[1] - 1.0) <= 1e-12
    p, _, info = gr.shape_vector(c, c, None, gr.as_params(3.0, "apg", eta=0.3, rho=1.0))
    assert info["tau"] == 1.0 and np.array_equal(p, c)
    # var_p == 0 (both branches 0, or constant): f = 1
    for cc_, uu_ in ((z, z), (np.full(N, 0.5), np.full(N, 0.5))):
        for mode in gr.MODES:
            co = gr.coefficients(gr.moments(cc_, uu_), N, gr.as_params(3.0, mode, phi=0.7))
            assert finite(co) and co[3] == 1.0, mode
            p, _, info = gr.shape_vector(cc_, uu_, None, gr.as_params(3.0, mode, phi=0.7))
            assert np.isfinite(p).all() and info["f"] == 1.0
    # everything zero, every mode, with r: no NaN
    for mode in gr.MODES:
        assert finite(gr.coefficients(np.zeros(9), N, gr.as_params(3.0, mode, phi=1.0, rho=1.0, mu=-0.5)))


def test_denoise_argument_check():
    from modules.flux_model import Flux

    chk = Flux._check_guidance_shaping
    assert chk(None, False, 1.0) is None and chk(None, True, 3.0) is None
    prm, off = chk(dict(mode="apg", rescale=0.5, eta=0.25, norm_threshold=10.0, momentum=-0.5, zero_init_steps=2, step_offset=3), True, 4.0)
    assert prm == [4.0, 0.5, 0.25, 10.0, -0.5, 1.0, 2.0, 0.0] and off == 3
    assert chk({}, True, 2.0) == ([2.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0], 0)
    for bad, msg in ((dict(mode="apg"), "needs a negative prompt"),):
        with pytest.raises(ValueError, match=msg):
            chk(bad, False, 3.0)
    for bad, msg in ((dict(mode="dynamic"), "unknown mode"), (dict(rescale=1.5), r"outside \[0, 1\]"), (dict(rescale=-0.1), r"outside \[0, 1\]"),
                     (dict(norm_threshold=-1.0), "must be >= 0"), (dict(zero_init_steps=-1), "must be >= 0"), (dict(step_offset=-2), "must be >= 0"),
                     (dict(eta=float("nan")), "finite"), (dict(scale=3.0), "expected a dict"), ("apg", "expected a dict")):
        with pytest.raises(ValueError, match=msg):
            chk(bad, True, 3.0)


def test_http_fields():
    import io

    from fastapi.testclient import TestClient

    import api

    calls = []

    class Stub:
        def generate(self, **kwargs):
            calls.append(kwargs)
            return io.BytesIO(b"jpeg")

    api.app.state.model = Stub()
    client = TestClient(api.app)
    assert client.post("/generate", json={"prompt": "a"}).status_code == 200
    assert not set(calls[-1]) & {"guidance_mode", "guidance_rescale", "apg_eta", "apg_norm_threshold", "apg_momentum", "zero_init_steps"}
    body = {"prompt": "a", "negative_prompt": "b", "true_cfg_scale": 4.0, "guidance_mode": "apg", "guidance_rescale": 0.5, "apg_eta": 0.0,
            "apg_norm_threshold": 15.0, "apg_momentum": -0.5, "zero_init_steps": 1}
    assert client.post("/generate", json=body).status_code == 200
    assert {k: calls[-1][k] for k in body} == body
    for bad in ({"guidance_mode": "dynamic"}, {"guidance_rescale": 1.5}, {"zero_init_steps": -1}, {"apg_norm_threshold": -1.0}):
        assert client.post("/generate", json={"prompt": "a", **bad}).status_code == 422
