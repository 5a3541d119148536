"""Higher-order samplers without a GPU: the host solver math (fluxmi/solvers.py) through the exact interpreter of tests/solver_util.py, the
schedules, and the arguments' way through FluxPipeline.generate / Flux.denoise / the HTTP surface.  Stubs are those of
tests/test_inpaint_cpu.py."""
import math
import os

import pytest
import torch

import solver_util as su
from test_inpaint_cpu import KW, H, W, box_mask, embeddings, make_pipe, photo

ORDER2 = ("heun", "midpoint", "ab2", "dpmpp_2m")
MU = 1.15  # the pipeline's shift at 4096 image tokens


def shift(t):
    return math.exp(MU) / (math.exp(MU) + (1.0 / t - 1.0)) if t > 0 else 0.0


def unshift(s):
    return 1.0 / (1.0 + math.exp(MU) * (1.0 / s - 1.0))


def grid(kind, N, end=0.05):
    """N steps from sigma = 1 to `end`: uniform, or the pipeline's shifted schedule (time_shift of a uniform ramp) cut at `end`"""
    if kind == "uniform":
        return [1.0 + (end - 1.0) * i / N for i in range(N)] + [end]
    u_end = unshift(end)
    return [1.0] + [shift(1.0 + (u_end - 1.0) * i / N) for i in range(1, N)] + [end]


# dx/dt = -x + sin(3 t):  x(t) = C exp(-t) + 0.1 sin(3 t) - 0.3 cos(3 t)
def field(x, t, j):
    return -x + math.sin(3.0 * t)


def closed_form(t, x1):
    p = lambda s: 0.1 * math.sin(3.0 * s) - 0.3 * math.cos(3.0 * s)
    return (x1 - p(1.0)) * math.e * math.exp(-t) + p(t)


def final_error(name, sig):
    from fluxmi import solvers

    x = su.run_program(solvers.build_program(name, sig), torch.tensor([0.7], dtype=torch.float64), field, exact=True)
    return abs(x.item() - closed_form(sig[-1], 0.7))


# ---- the mathematics --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "shifted"])
def test_convergence_order(kind):
    """N = 64 against 2N = 128 steps: measured on the host, every solver is in its asymptotic regime there (the ratios of the order-2
    solvers lie between 3.76 and 4.06 on both grids, Euler's between 1.92 and 2.01; at N = 16 dpmpp_2m on the shifted grid is not yet)"""
    from fluxmi import solvers

    for name in solvers.SAMPLERS:
        e1, e2 = final_error(name, grid(kind, 64)), final_error(name, grid(kind, 128))
        ratio = e1 / e2
        print(f"[{kind}] {name}: error {e1:.3e} at N = 64, {e2:.3e} at N = 128, ratio {ratio:.2f}")
        if name == "euler":
            assert 1.6 <= ratio <= 2.4, f"{name} on the {kind} grid: error ratio {ratio:.2f} outside [1.6, 2.4]"
        else:
            assert ratio >= 3.0, f"{name} on the {kind} grid: error ratio {ratio:.2f} < 3 (order 2 gives 4)"
            assert e1 < final_error("euler", grid(kind, 64))


def test_euler_program_is_the_plain_recurrence():
    from fluxmi import solvers

    for sig in (grid("shifted", 24), grid("shifted", 24, end=0.3)[:-1] + [0.0], grid("uniform", 7)):
        x0 = torch.tensor([0.7, -1.3], dtype=torch.float64)
        got = su.run_program(solvers.build_program("euler", sig), x0, field, exact=True)
        x = x0.clone()
        for a, b in zip(sig[:-1], sig[1:]):
            x = x + (b - a) * field(x, a, 0)
        assert (got - x).abs().max().item() <= 1e-12


# ---- the structure of the programs --------------------------------------------------------------------------------------------------------
def test_program_structure():
    from fluxmi import solvers

    N = 6
    ends_at_0 = grid("shifted", N, end=0.2)[:-1] + [0.0]
    for sig in (grid("shifted", N), ends_at_0):
        for name in solvers.SAMPLERS:
            p = solvers.build_program(name, sig)
            n = len(p.coef)
            assert len(p.ctl) == n and len(p.step_of_eval) == n and len(p.times) == n + 1 and p.times[-1] == sig[-1]
            assert all(len(r) == 8 and r[7] == 0.0 for r in p.coef) and all(len(c) == 4 for c in p.ctl)
            assert all(math.isfinite(v) for r in p.coef for v in r)
            # monotone, covers 0 .. N - 1
            assert list(p.step_of_eval) == sorted(p.step_of_eval) and set(p.step_of_eval) == set(range(N))
            # every evaluation's time is its user step's start or inside the step; the produced iterates' times never rise
            assert all(sig[i] >= p.times[j] >= sig[i + 1] for j, i in enumerate(p.step_of_eval))
            # no slot, and no saved iterate, is read before it is written
            written, saved = set(), False
            for row, (save, w, h1, h2) in zip(p.coef, p.ctl):
                assert all(s in (-1, 0, 1) for s in (w, h1, h2))
                if row[1] != 0.0:
                    assert saved, f"{name}: xs read before it is saved"
                if row[3] != 0.0:
                    assert h1 in written, f"{name}: slot {h1} read before it is written"
                if row[4] != 0.0:
                    assert h2 in written, f"{name}: slot {h2} read before it is written"
                saved = saved or bool(save)
                if w >= 0:
                    written.add(w)
    # Heun: 2N - 1 evaluations at t0, t1, t1, t2, t2, ... (diffusers' FlowMatchHeunDiscreteScheduler), the last step first-order
    for sig in (grid("shifted", N), ends_at_0):
        p = solvers.build_program("heun", sig)
        assert len(p.coef) == 2 * N - 1
        assert list(p.times) == [sig[0]] + [t for t in sig[1:N] for _ in (0, 1)] + [sig[N]]
        assert list(p.step_of_eval) == [i for i in range(N - 1) for _ in (0, 1)] + [N - 1]
    # midpoint: evaluations at t_i and t_i + dt / 2
    p = solvers.build_program("midpoint", grid("uniform", N))
    sig = grid("uniform", N)
    assert len(p.coef) == 2 * N and all(p.times[2 * i] == sig[i] and abs(p.times[2 * i + 1] - 0.5 * (sig[i] + sig[i + 1])) < 1e-15 for i in range(N))
    for name in ("euler", "ab2", "dpmpp_2m"):
        assert len(solvers.build_program(name, sig).coef) == N
    # a schedule that ends at 0: the last evaluation of every solver produces exactly D = x - sigma v (cx == 0)
    x, v = torch.tensor([0.37, -2.5], dtype=torch.float64), torch.tensor([1.9, 0.4], dtype=torch.float64)
    for name in solvers.SAMPLERS:
        p = solvers.build_program(name, ends_at_0)
        assert p.coef[-1][0] == 0.0 and p.coef[-1][1] == 0.0 and p.coef[-1][3] == 0.0 and p.coef[-1][4] == 0.0
        xs, hist = su.new_state(x, exact=True, fill=float("nan"))
        got = su.apply_row(x, v, p.coef[-1], p.ctl[-1], xs, hist, exact=True)
        assert torch.equal(got, x - p.times[-2] * v) and p.times[-2] == ends_at_0[-2]


def test_dpmpp_2m_coefficients():
    """cx = s_{i+1} / s_i; c0 = (1 - cx)(1 + 1 / (2 r)), c1 = -(1 - cx) / (2 r), r = (l_i - l_{i-1}) / (l_{i+1} - l_i), l = -log s; the first step
    has c1 = 0; and a constant data prediction is integrated exactly"""
    from fluxmi import solvers

    sig = grid("shifted", 5)
    p = solvers.build_program("dpmpp_2m", sig)
    lam = [-math.log(s) for s in sig]
    for i, row in enumerate(p.coef):
        cx = sig[i + 1] / sig[i]
        assert row[0] == cx and row[5] == 1.0 and row[6] == -sig[i]
        if i == 0:
            assert row[2] == 1.0 - cx and row[3] == 0.0
        else:
            r = (lam[i] - lam[i - 1]) / (lam[i + 1] - lam[i])
            assert abs(row[2] - (1 - cx) * (1 + 1 / (2 * r))) < 1e-15 and abs(row[3] + (1 - cx) / (2 * r)) < 1e-15
    data, eps = torch.tensor([0.3], dtype=torch.float64), torch.tensor([-1.1], dtype=torch.float64)
    for name in solvers.SAMPLERS:  # v = eps - data is constant along the straight path: every solver lands on it
        got = su.run_program(solvers.build_program(name, sig), (1 - sig[0]) * data + sig[0] * eps, lambda x, t, j: eps - data, exact=True)
        assert abs(got.item() - ((1 - sig[-1]) * data + sig[-1] * eps).item()) < 1e-14


# ---- schedules ------------------------------------------------------------------------------------------------------------------------------
def test_sigma_schedule():
    from fluxmi import solvers

    base = grid("shifted", 12, end=0.04)[:-1] + [0.04, 0.0]
    assert solvers.sigma_schedule(None, base) == base
    for kind in ("karras", "exponential"):
        s = solvers.sigma_schedule(kind, base)
        assert len(s) == len(base) and s[0] == base[0] and s[-2] == base[-2] and s[-1] == 0.0
        assert all(a > b for a, b in zip(s[:-1], s[1:])) and s != base
        t = solvers.sigma_schedule(kind, base[:-1])  # no trailing 0: none appended
        assert t == s[:-1]
    k = solvers.sigma_schedule("karras", base)
    rho = 7.0
    a, b, n = base[0] ** (1 / rho), base[-2] ** (1 / rho), len(base) - 1
    assert all(abs(k[i] - (a + i / (n - 1) * (b - a)) ** rho) < 1e-15 for i in range(n))
    e = solvers.sigma_schedule("exponential", base)
    assert all(abs(math.log(e[i]) - (math.log(base[0]) + i / (n - 1) * (math.log(base[-2]) - math.log(base[0])))) < 1e-14 for i in range(n))
    with pytest.raises(ValueError, match="sigma_schedule"):
        solvers.sigma_schedule("cosine", base)


def test_malformed_sigmas_and_unknown_samplers_are_refused():
    from fluxmi import solvers

    assert solvers.custom_sigmas([1.0, 0.5, 0.25]) == [1.0, 0.5, 0.25, 0.0]
    assert solvers.custom_sigmas([0.9, 0.5, 0.0]) == [0.9, 0.5, 0.0]
    for bad in ([], [0.0], [1.0, 1.0, 0.5], [0.5, 0.75], [1.5, 0.5], [1.0, float("nan")], [1.0, float("inf")], [1.0, -0.5], [1.0, 0.0, 0.0],
                ["a"], [1.0, 0.5, 0.0, 0.25]):
        with pytest.raises(ValueError):
            solvers.custom_sigmas(bad)
    with pytest.raises(ValueError, match="sampler"):
        solvers.build_program("rk4", [1.0, 0.5, 0.0])
    with pytest.raises(ValueError, match="descending"):
        solvers.build_program("heun", [0.5, 1.0])


# ---- the arguments' way through the pipeline ------------------------------------------------------------------------------------------------
def test_generate_builds_the_program_from_the_final_timesteps():
    from fluxmi import solvers

    pipe = make_pipe()
    pos = embeddings(1, 3)
    base = pipe.generate(pos, **KW)
    assert "solver" not in pipe.model.calls[-1]
    ts = pipe.model.calls[-1]["ts"]
    assert len(ts) == KW["num_steps"] + 1
    # sampler="euler" with no other new argument is today's call
    assert torch.equal(pipe.generate(pos, sampler="euler", **KW), base) and "solver" not in pipe.model.calls[-1]
    assert pipe.model.calls[-1]["ts"] == ts
    for name in ("heun", "midpoint", "ab2", "dpmpp_2m"):
        pipe.generate(pos, sampler=name, **KW)
        c = pipe.model.calls[-1]
        assert c["ts"] == ts and c["solver"] == solvers.build_program(name, ts)
    # a sigma schedule re-spaces the request's own list; the program follows it
    pipe.generate(pos, sampler="dpmpp_2m", sigma_schedule="karras", **KW)
    c = pipe.model.calls[-1]
    assert c["ts"] == solvers.sigma_schedule("karras", ts) and c["solver"] == solvers.build_program("dpmpp_2m", c["ts"])
    pipe.generate(pos, sigma_schedule="exponential", **KW)  # ... with Euler too, which takes no program
    assert pipe.model.calls[-1]["ts"] == solvers.sigma_schedule("exponential", ts) and "solver" not in pipe.model.calls[-1]
    # sigmas= replaces the schedule and num_steps follows its length, with or without the trailing 0
    mine = [1.0, 0.8, 0.55, 0.2]
    for given in (mine, mine + [0.0]):
        pipe.generate(pos, sampler="heun", sigmas=given, **KW)
        c = pipe.model.calls[-1]
        assert c["ts"] == mine + [0.0] and len(c["solver"].coef) == 2 * 4 - 1
    # img2img: the program is built from the truncated list
    pipe.generate(pos, sampler="ab2", init_image=photo(), strength=0.5, **KW)
    c = pipe.model.calls[-1]
    assert c["ts"] == ts[4:] and c["solver"] == solvers.build_program("ab2", ts[4:])
    # differential inpainting: the thresholds stay one per USER step (Flux.denoise expands them per evaluation)
    pipe.generate(pos, sampler="heun", init_image=photo(), inpaint_mask=box_mask(), inpaint_differential=True, **KW)
    c = pipe.model.calls[-1]
    assert len(c["inpaint_thresholds"]) == KW["num_steps"] and len(c["solver"].coef) == 2 * KW["num_steps"] - 1
    # refusals, before the flow model is reached
    n = len(pipe.model.calls)
    with pytest.raises(ValueError, match="sampler"):
        pipe.generate(pos, sampler="rk4", **KW)
    with pytest.raises(ValueError, match="sigma_schedule"):
        pipe.generate(pos, sigma_schedule="cosine", **KW)
    with pytest.raises(ValueError, match="descending"):
        pipe.generate(pos, sigmas=[0.5, 0.75], **KW)
    with pytest.raises(ValueError, match="cache_threshold"):
        pipe.generate(pos, sampler="heun", cache_threshold=0.1, **KW)
    assert len(pipe.model.calls) == n
    pipe.generate(pos, sampler="euler", cache_threshold=0.1, **KW)  # Euler keeps the step cache
    assert pipe.model.calls[-1]["cache_threshold"] == 0.1


def tiny_cpu_model():
    import util
    from fluxmi import synth

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    p = cfg.params
    p.hidden_size, p.num_heads, p.depth, p.depth_single_blocks, p.context_in_dim, p.vec_in_dim = 256, 2, 1, 1, 128, 64
    return util.load_flow_model(cfg, synth.make_state_dict(p, seed=0))


def test_denoise_refuses_a_solver_with_step_caching_before_any_device_work():
    from fluxmi import solvers

    model = tiny_cpu_model()
    B, Li, Lt = 2, 4, 6
    img, ids = torch.zeros(B, Li, 64), torch.zeros(B, Li, 3)
    txt, tids, y = torch.zeros(B, Lt, 128), torch.zeros(B, Lt, 3), torch.zeros(B, 64)
    ts = [1.0, 0.5, 0.0]
    with pytest.raises(ValueError, match="cache_threshold"):
        model.denoise(img, ids, txt, tids, y, ts, solver=solvers.build_program("heun", ts), cache_threshold=0.1)
    with pytest.raises(ValueError, match="solver"):  # a program built from another list
        model.denoise(img, ids, txt, tids, y, ts, solver=solvers.build_program("heun", [1.0, 0.7, 0.4, 0.0]))
    with pytest.raises(ValueError, match="solver"):  # ... or from another list of the same length
        model.denoise(img, ids, txt, tids, y, ts, solver=solvers.build_program("heun", [0.9, 0.4, 0.0]))
    with pytest.raises(ValueError, match="solver"):
        model.denoise(img, ids, txt, tids, y, ts, solver=solvers.build_program("midpoint", [1.0, 0.5, 0.1]))
    assert model._engine is None, "a refused request created the engine"


def test_chunked_batches_carry_the_solver():
    from fluxmi import solvers

    model = tiny_cpu_model()
    model.MAX_ENGINE_BATCH = 2
    whole, calls = model.denoise, []

    def single_pass(img, img_ids, txt, txt_ids, y, timesteps, **kw):
        if img.shape[0] > 2:
            return whole(img, img_ids, txt, txt_ids, y, timesteps, **kw)
        calls.append(dict(kw, ts=list(timesteps)))
        return img + 1

    model.denoise = single_pass
    B, Li, Lt = 5, 4, 6
    img, ids = torch.zeros(B, Li, 64), torch.zeros(B, Li, 3)
    txt, tids, y = torch.zeros(B, Lt, 128), torch.zeros(B, Lt, 3), torch.zeros(B, 64)
    ts = [1.0, 0.5, 0.0]
    prog = solvers.build_program("heun", ts)
    model.denoise(img, ids, txt, tids, y, ts, solver=prog)
    assert len(calls) == 3 and all(c["solver"] is prog and c["ts"] == ts for c in calls)
    calls.clear()
    model.denoise(img, ids, txt, tids, y, ts)
    assert len(calls) == 3 and not any("solver" in c for c in calls)


# ---- the interfaces ---------------------------------------------------------------------------------------------------------------------
def test_ctypes_table_has_the_solver_entries():
    from fluxmi import _lib

    assert "fluxmi_solver_step" in _lib.EXPORTS and "fluxmi_engine_set_solver" in _lib.EXPORTS
    assert len(_lib.lib.fluxmi_solver_step.argtypes) == len(_lib.lib.fluxmi_blend_euler.argtypes) + 3  # + xs, hist, coef, ctl - dts
    assert len(_lib.lib.fluxmi_engine_set_solver.argtypes) == 4
    assert _lib.lib.fluxmi_abi_version() == 5 and _lib.ABI_VERSION == 5
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "fluxmi.h")).read()
    assert "int fluxmi_solver_step(" in header and "int fluxmi_engine_set_solver(" in header


def test_http_sampler_fields():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient

    import api

    seen = {}

    class Stub:
        def generate(self, **kw):
            import io

            seen.clear()
            seen.update(kw)
            return io.BytesIO(b"jpeg")

    api.app.state.model = Stub()
    client = TestClient(api.app)
    assert client.post("/generate", json={"prompt": "a"}).status_code == 200
    assert not any(k in seen for k in ("sampler", "sigma_schedule", "sigmas"))
    r = client.post("/generate", json={"prompt": "a", "sampler": "dpmpp_2m", "sigma_schedule": "karras", "sigmas": [1.0, 0.5, 0.25]})
    assert r.status_code == 200 and seen["sampler"] == "dpmpp_2m" and seen["sigma_schedule"] == "karras" and seen["sigmas"] == [1.0, 0.5, 0.25]
    assert client.post("/generate", json={"prompt": "a", "sampler": "rk4"}).status_code == 422
    assert client.post("/generate", json={"prompt": "a", "sigma_schedule": "cosine"}).status_code == 422
