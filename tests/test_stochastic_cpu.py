"""Stochastic samplers without a GPU: the numpy Philox reference against published known answers, the host programs of
fluxmi/solvers.py (euler_ancestral, dpmpp_2m_sde) in float64, the interpreter's noise term, and the arguments' way through
FluxPipeline.generate / Flux.denoise / the HTTP surface.  Stubs are those of tests/test_inpaint_cpu.py and tests/test_solvers_cpu.py."""
import math
import os

import numpy as np
import pytest
import torch

import inpaint_util as iu
import solver_util as su
import stochastic_util as st
from test_inpaint_cpu import KW, StubFlow, box_mask, embeddings, make_pipe, photo
from test_solvers_cpu import field, grid, tiny_cpu_model

ETAS = (0.0, 0.3, 1.0)
STEPS = (4, 12, 28)


def schedules():
    """shifted schedules from sigma = 1: ending above 0, and ending at 0"""
    for n in STEPS:
        yield grid("shifted", n)
        yield grid("shifted", n, end=0.2)[:-1] + [0.0]


# ---- the generator ----------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds: counter / key -> output"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = tuple(int(v) for v in st.philox4x32_10(ctr, key))
        assert got == want, f"{ctr} / {key}: {[hex(v) for v in got]}"
    # the vectorised form is the scalar one per block, and the layout is (q, eval, c2, c3) / (key_lo, key_hi)
    ids = (0xa4093822, 0x299f31d0, 0x13198a2e, 0x03707344)
    w = st.words(ids, 32, 0x85a308d3)
    for q in range(8):
        assert tuple(w[4 * q:4 * q + 4]) == tuple(st.philox4x32_10((q, 0x85a308d3, ids[2], ids[3]), ids[:2]))
    assert w.dtype == np.uint32 and len(set(w.tolist())) == 32


def test_box_muller_reference():
    """u in (0, 1) and t in [0, 1) at the extreme words: finite normals, |z| <= sqrt(-2 log(2^-24)) < 5.77; moments of a real draw"""
    edge = st.normals64(np.array([0, 0, 0xffffffff, 0xffffffff, 0, 0xffffffff, 0xffffffff, 0], dtype=np.uint32))
    assert np.isfinite(edge).all() and np.abs(edge).max() < 5.77
    z = st.normals64(st.words(st.ids_of(1234567890123, 3), 1 << 16, 5))
    # 65536 normals: the mean's standard error is 0.0039, the variance's 0.0055: six of them
    assert abs(z.mean()) < 6 * 0.0039 and abs(z.var() - 1.0) < 6 * 0.0055
    # another evaluation, image or seed: another stream
    base = st.words(st.ids_of(7, 0), 64, 0)
    for other in (st.words(st.ids_of(7, 0), 64, 1), st.words(st.ids_of(7, 1), 64, 0), st.words(st.ids_of(8, 0), 64, 0),
                  st.words(st.ids_of(7 + (1 << 32), 0), 64, 0)):
        assert not np.array_equal(base, other)


# ---- the programs -----------------------------------------------------------------------------------------------------------------------
def carried(p, sig):
    """every row on x = (1 - a) x0 + a eps, v = eps - x0 (so D = x0), history slots holding what earlier rows of the same kind wrote:
    x' = A x0 + B eps + cn z -> [(A, B, cn, b)]"""
    out, slots = [], {}
    for j, (row, (save, w, h1, h2)) in enumerate(zip(p.coef, p.ctl)):
        a, b = sig[j], sig[j + 1]
        cx, cs, c0, c1, c2, ga, gb, cn = row
        assert cs == 0.0 and c2 == 0.0 and not save
        g = (ga * (1.0 - a) - gb, ga * a + gb)
        h = slots[h1] if c1 != 0.0 else (0.0, 0.0)
        out.append((cx * (1.0 - a) + c0 * g[0] + c1 * h[0], cx * a + c0 * g[1] + c1 * h[1], cn, b))
        if w >= 0:
            slots[w] = g
    return out


def test_programs_carry_the_marginals():
    """|A - (1 - b)| <= 1e-12 and |B^2 + cn^2 - b^2| <= 1e-12 for every row, a first sigma of 1 included"""
    from fluxmi import solvers

    worst = 0.0
    for sig in schedules():
        assert sig[0] == 1.0
        for eta in ETAS:
            for s_noise in (1.0,):
                for name in solvers.STOCHASTIC_SAMPLERS:
                    p = solvers.build_program(name, sig, eta, s_noise)
                    for j, (A, B, cn, b) in enumerate(carried(p, sig)):
                        e = max(abs(A - (1.0 - b)), abs(B * B + cn * cn - b * b))
                        worst = max(worst, e)
                        assert e <= 1e-12, f"{name} eta={eta} N={len(sig) - 1} row {j}: A {A} B {B} cn {cn} b {b}"
    print(f"worst identity error {worst:.3e}")
    # s_noise scales cn and nothing else
    sig = grid("shifted", 12)
    for name in solvers.STOCHASTIC_SAMPLERS:
        p1, p2 = solvers.build_program(name, sig, 0.7, 1.0), solvers.build_program(name, sig, 0.7, 0.5)
        assert all(r1[:7] == r2[:7] and r2[7] == 0.5 * r1[7] for r1, r2 in zip(p1.coef, p2.coef)) and p1.ctl == p2.ctl
        assert all(r[7] == 0.0 for r in solvers.build_program(name, sig, 0.7, 0.0).coef)


def test_eta_zero_is_deterministic():
    from fluxmi import solvers

    for sig in schedules():
        for name in solvers.STOCHASTIC_SAMPLERS:
            p = solvers.build_program(name, sig, eta=0.0)
            assert all(r[7] == 0.0 for r in p.coef) and not solvers.has_noise(p)
        # euler_ancestral at eta 0 is the Euler recurrence
        x0 = torch.tensor([0.7, -1.3], dtype=torch.float64)
        got = su.run_program(solvers.build_program("euler_ancestral", sig, eta=0.0), x0, field, exact=True)
        x = x0.clone()
        for a, b in zip(sig[:-1], sig[1:]):
            x = x + (b - a) * field(x, a, 0)
        assert (got - x).abs().max().item() <= 1e-12
        # dpmpp_2m_sde at eta 0: the coefficients of x and of the D's are dpmpp_2m's sums
        p = solvers.build_program("dpmpp_2m_sde", sig, eta=0.0)
        for j, row in enumerate(p.coef):
            a, b = sig[j], sig[j + 1]
            if b == 0.0:
                continue
            assert abs(row[0] - b / a) <= 1e-15 and abs(row[2] + row[3] - (1.0 - b / a)) <= 1e-15, f"N={len(sig) - 1} row {j}: {row}"


def test_stochastic_program_structure():
    from fluxmi import solvers

    for sig in schedules():
        N = len(sig) - 1
        for eta in ETAS:
            for name in solvers.STOCHASTIC_SAMPLERS:
                p = solvers.build_program(name, sig, eta)
                assert len(p.coef) == N and len(p.ctl) == N and list(p.step_of_eval) == list(range(N)) and list(p.times) == sig
                assert all(len(r) == 8 and all(math.isfinite(v) for v in r) for r in p.coef) and all(len(c) == 4 for c in p.ctl)
                assert all(r[7] >= 0.0 for r in p.coef) and (eta == 0.0 or solvers.has_noise(p))
                written = set()
                for row, (save, w, h1, h2) in zip(p.coef, p.ctl):
                    assert all(s in (-1, 0, 1) for s in (w, h1, h2)) and not save and row[1] == 0.0 and row[4] == 0.0 and h2 == -1
                    if row[3] != 0.0:
                        assert h1 in written, f"{name}: slot {h1} read before it is written"
                    if w >= 0:
                        written.add(w)
                if name == "euler_ancestral":
                    assert all(c == (0, -1, -1, -1) for c in p.ctl)
                elif N > 2:  # the multistep rows read the slot the row before wrote; the row behind sigma = 1 has no usable history
                    assert p.coef[1][3] == 0.0 and p.ctl[1][2] == -1
                    assert all(p.coef[j][3] != 0.0 and p.ctl[j][2] == p.ctl[j - 1][1] for j in range(2, N) if sig[j + 1] != 0.0)
                if sig[-1] == 0.0:  # onto sigma 0: the deterministic x' = D row
                    assert p.coef[-1] == (0.0, 0.0, 1.0, 0.0, 0.0, 1.0, -sig[-2], 0.0) and p.ctl[-1] == (0, -1, -1, -1)
                    assert p.coef[-1] == solvers.build_program("euler", sig).coef[-1]
    # a schedule that does not start at 1: the second row of dpmpp_2m_sde is already a multistep row
    p = solvers.build_program("dpmpp_2m_sde", [0.9, 0.6, 0.3, 0.1], 0.5)
    assert p.coef[1][3] != 0.0 and p.ctl[1][2] == 0 and p.ctl[0][1] == 0
    # SAMPLERS stays the deterministic list, and every deterministic program ignores eta / s_noise
    assert solvers.SAMPLERS == ("euler", "heun", "midpoint", "ab2", "dpmpp_2m") and solvers.STOCHASTIC_SAMPLERS == ("euler_ancestral", "dpmpp_2m_sde")
    for name in solvers.SAMPLERS:
        assert solvers.build_program(name, grid("shifted", 6), 0.3, 2.0) == solvers.build_program(name, grid("shifted", 6))


def test_bad_eta_s_noise_and_names_are_refused():
    from fluxmi import solvers

    sig = [1.0, 0.5, 0.0]
    for name in solvers.STOCHASTIC_SAMPLERS:
        for eta in (-0.01, 1.01, float("nan"), float("inf"), "much"):
            with pytest.raises(ValueError, match="eta"):
                solvers.build_program(name, sig, eta=eta)
        for s_noise in (-0.5, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="s_noise"):
                solvers.build_program(name, sig, s_noise=s_noise)
        with pytest.raises(ValueError, match=r"\(0, 1\]"):
            solvers.build_program(name, [1.5, 0.5, 0.0])
        with pytest.raises(ValueError, match="descending"):
            solvers.build_program(name, [0.5, 1.0])
    for name in ("euler_a", "dpmpp_sde", "Euler_Ancestral"):
        with pytest.raises(ValueError, match="sampler"):
            solvers.build_program(name, sig)


# ---- the interpreter --------------------------------------------------------------------------------------------------------------------
def test_interpreter_without_noise_is_solver_utils():
    g = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16)
    shape = (2, 5, 16)
    rows = [((0.75, 0.3, -0.0625, 0.41, -0.17, 0.9, -0.6, 0.0), (1, 1, 0, 1)), ((1.0, 0.0, -0.03, 0.0, 0.0, 0.0, 1.0, 0.0), (0, -1, -1, -1)),
            ((0.0, 0.0, 1.0, 0.5, 0.25, 1.0, -0.7, 0.0), (0, 0, -1, -1)), ((0.0,) * 8, (0, -1, -1, -1))]
    for row, ctl in rows:
        for guided in (False, True):
            for blend in (None, "linear", "differential"):
                x, v, u = rnd(*shape), rnd(*shape), rnd(*shape)
                xs, hist = rnd(*shape), torch.randn(2, *shape, generator=g)
                bl = None if blend is None else (rnd(*shape), rnd(*shape), torch.rand(*shape, generator=g).to(torch.bfloat16), 0.4,
                                                 0.5 if blend == "differential" else None)
                a_xs, a_h, b_xs, b_h = xs.clone(), hist.clone(), xs.clone(), hist.clone()
                kw = dict(scale=2.5 if guided else None, blend=bl)
                a = su.apply_row(x, (v, u) if guided else v, row, ctl, a_xs, a_h, **kw)
                b = st.apply_row(x, (v, u) if guided else v, row, ctl, b_xs, b_h, z=None, **kw)
                assert torch.equal(a, b) and torch.equal(a_xs, b_xs) and torch.equal(a_h, b_h)
    # the noise term comes last: acc + cn * z with the product rounded on its own, before the one bf16 store
    x, v, z = rnd(*shape), rnd(*shape), torch.randn(*shape, generator=g)
    row = (0.75, 0.0, 0.2, 0.0, 0.0, 1.0, -0.6, 0.37)
    xs, hist = su.new_state(x)
    got = st.apply_row(x, v, row, (0, -1, -1, -1), xs, hist, z=z)
    X, V, f = x.float(), v.float(), su.f32
    want = (X * f(0.75) + (X * f(1.0) + V * f(-0.6)) * f(0.2) + z * f(0.37)).to(torch.bfloat16)
    assert torch.equal(got, want) and not torch.equal(got, st.apply_row(x, v, row[:7] + (0.0,), (0, -1, -1, -1), xs, hist))


# ---- the arguments' way through the pipeline ------------------------------------------------------------------------------------------------
class CheckingFlow(StubFlow):
    """the recording stub, behind the checks the real Flux.denoise makes of (solver, solver_noise) before any device work"""

    def denoise(self, img, img_ids, txt, txt_ids, vec, timesteps, **kw):
        from modules.flux_model import Flux

        Flux._check_solver_noise(kw.get("solver_noise"), kw.get("solver"), img.shape[0])
        return super().denoise(img, img_ids, txt, txt_ids, vec, timesteps, **kw)


def test_slices_that_draw_nothing_carry_no_ids():
    """eta = 0, s_noise = 0, a one-step request and a cut whose last slice is only the step onto sigma 0: their programs have no non-zero
    cn, Flux.denoise and the engine refuse ids with such a program, so generate passes none -- and keeps counting the evaluations"""
    from fluxmi import solvers

    pipe = make_pipe(CheckingFlow())
    pos, neg = embeddings(1, 3), embeddings(1, 4)
    seed = KW["seed"]
    for name in solvers.STOCHASTIC_SAMPLERS:
        for req in (dict(eta=0.0), dict(s_noise=0.0), dict(num_steps=1)):
            pipe.generate(pos, sampler=name, **dict(KW, **req))
            c = pipe.model.calls[-1]
            assert "solver_noise" not in c and not solvers.has_noise(c["solver"]), f"{name} {req}"
            assert c["solver"] == solvers.build_program(name, c["ts"], req.get("eta", 1.0), req.get("s_noise", 1.0))
        # 8 steps, guided on [0, 7): the last slice is the single deterministic step onto 0
        n0 = len(pipe.model.calls)
        pipe.generate(pos, sampler=name, negative_prompt=neg, true_cfg_scale=3.5, true_cfg_interval=(0.0, 0.875), **KW)
        calls = pipe.model.calls[n0:]
        assert [len(c["ts"]) - 1 for c in calls] == [7, 1] and calls[1]["ts"][-1] == 0.0
        assert calls[0]["solver_noise"] == ([(seed, 0, 0, 0)], 0) and "solver_noise" not in calls[1]
        assert calls[1]["solver"].coef[0][7] == 0.0
        # a cut in the middle: the slice behind a noiseless-free head still starts at its own evaluation index
        n0 = len(pipe.model.calls)
        pipe.generate(pos, sampler=name, negative_prompt=neg, true_cfg_scale=3.5, true_cfg_interval=(0.5, 0.875), **KW)
        calls = pipe.model.calls[n0:]
        assert [len(c["ts"]) - 1 for c in calls] == [4, 3, 1]
        assert [c.get("solver_noise", (None, None))[1] for c in calls] == [0, 4, None]
    # the real checks do refuse what generate used to pass
    from modules.flux_model import Flux

    for prog in (solvers.build_program("euler_ancestral", [1.0, 0.5, 0.2], eta=0.0), solvers.build_program("dpmpp_2m_sde", [1.0, 0.5, 0.2], s_noise=0.0),
                 solvers.build_program("euler_ancestral", [0.3, 0.0]), solvers.build_program("dpmpp_2m_sde", [1.0, 0.0])):
        assert Flux._check_solver_noise(None, prog, 1) is None
        with pytest.raises(ValueError, match="solver_noise"):
            Flux._check_solver_noise(([(1, 0, 0, 0)], 0), prog, 1)


def test_generate_passes_the_program_ids_and_offsets():
    from fluxmi import solvers

    pipe = make_pipe(CheckingFlow())
    pos = embeddings(1, 3)
    base = pipe.generate(pos, **KW)
    ts = pipe.model.calls[-1]["ts"]
    assert "solver_noise" not in pipe.model.calls[-1]
    seed = KW["seed"]
    for name in solvers.STOCHASTIC_SAMPLERS:
        pipe.generate(pos, sampler=name, **KW)
        c = pipe.model.calls[-1]
        assert c["ts"] == ts and c["solver"] == solvers.build_program(name, ts, 1.0, 1.0) and solvers.has_noise(c["solver"])
        assert c["solver_noise"] == ([(seed, 0, 0, 0)], 0)
        pipe.generate(pos, sampler=name, eta=0.5, s_noise=0.9, noise_seed=(5 << 32) + 9, num_images=3, **KW)
        c = pipe.model.calls[-1]
        assert c["solver"] == solvers.build_program(name, ts, 0.5, 0.9)
        assert c["solver_noise"] == ([(9, 5, k, 0) for k in range(3)], 0)
    # nothing is drawn from the request's generator: the initial latents are the deterministic request's
    pipe.generate(pos, **KW)
    first = pipe.model.calls[-1]["img"]
    pipe.generate(pos, sampler="euler_ancestral", noise_seed=99, **KW)
    assert torch.equal(pipe.model.calls[-1]["img"], first)
    # a request cut by true_cfg_interval: each slice's program, and the evaluations before it as its offset
    n0 = len(pipe.model.calls)
    pipe.generate(pos, sampler="dpmpp_2m_sde", eta=0.5, negative_prompt=embeddings(1, 4), true_cfg_scale=3.5, true_cfg_interval=(0.25, 0.75), **KW)
    calls = pipe.model.calls[n0:]
    assert [len(c["ts"]) - 1 for c in calls] == [2, 4, 2]
    assert [c["solver_noise"][1] for c in calls] == [0, 2, 6]
    assert all(c["solver_noise"][0] == [(seed, 0, 0, 0)] for c in calls)
    assert [c["solver"] for c in calls] == [solvers.build_program("dpmpp_2m_sde", ts[a:b + 1], 0.5) for a, b in ((0, 2), (2, 6), (6, 8))]
    # img2img and inpainting compose: the program of the truncated list, offsets from its start
    pipe.generate(pos, sampler="euler_ancestral", init_image=photo(), strength=0.5, inpaint_mask=box_mask(), **KW)
    c = pipe.model.calls[-1]
    assert c["ts"] == ts[4:] and c["solver"] == solvers.build_program("euler_ancestral", ts[4:]) and c["solver_noise"][1] == 0
    # refusals, before the flow model is reached
    n = len(pipe.model.calls)
    for bad in (dict(sampler="euler_ancestral", cache_threshold=0.1), dict(sampler="dpmpp_2m_sde", cache_threshold=0.1)):
        with pytest.raises(ValueError, match="cache_threshold"):
            pipe.generate(pos, **bad, **KW)
    for bad in (dict(eta=0.5), dict(s_noise=0.5), dict(noise_seed=3), dict(sampler="heun", eta=0.0), dict(sampler="dpmpp_2m", s_noise=2.0)):
        with pytest.raises(ValueError, match="stochastic sampler"):
            pipe.generate(pos, **bad, **KW)
    with pytest.raises(ValueError, match="eta"):
        pipe.generate(pos, sampler="euler_ancestral", eta=1.5, **KW)
    with pytest.raises(ValueError, match="s_noise"):
        pipe.generate(pos, sampler="euler_ancestral", s_noise=-1.0, **KW)
    for bad in (-1, 1 << 64, 1.5, "7"):
        with pytest.raises(ValueError, match="noise_seed"):
            pipe.generate(pos, sampler="euler_ancestral", noise_seed=bad, **KW)
    with pytest.raises(ValueError, match="sampler"):
        pipe.generate(pos, sampler="euler_a", **KW)
    assert len(pipe.model.calls) == n
    # the deterministic calls are untouched
    assert torch.equal(pipe.generate(pos, sampler="euler", **KW), base) and "solver" not in pipe.model.calls[-1]
    pipe.generate(pos, sampler="heun", **KW)
    assert "solver_noise" not in pipe.model.calls[-1]


def test_denoise_checks_solver_noise_before_any_device_work():
    from fluxmi import solvers

    model = tiny_cpu_model()
    B, Li, Lt = 2, 4, 6
    img, ids = torch.zeros(B, Li, 64), torch.zeros(B, Li, 3)
    txt, tids, y = torch.zeros(B, Lt, 128), torch.zeros(B, Lt, 3), torch.zeros(B, 64)
    ts = [1.0, 0.5, 0.0]
    prog = solvers.build_program("euler_ancestral", ts)
    good = [(1, 2, 0, 0), (1, 2, 1, 0)]
    with pytest.raises(ValueError, match="solver_noise"):  # a program that draws, and no ids
        model.denoise(img, ids, txt, tids, y, ts, solver=prog)
    with pytest.raises(ValueError, match="solver_noise"):  # ids, and a program that draws nothing
        model.denoise(img, ids, txt, tids, y, ts, solver=solvers.build_program("heun", ts), solver_noise=(good, 0))
    with pytest.raises(ValueError, match="solver_noise"):
        model.denoise(img, ids, txt, tids, y, ts, solver=solvers.build_program("euler_ancestral", ts, eta=0.0), solver_noise=(good, 0))
    with pytest.raises(ValueError, match="solver_noise"):
        model.denoise(img, ids, txt, tids, y, ts, solver_noise=(good, 0))
    for bad in ((good[:1], 0), ([(1, 2, 0), (1, 2, 1)], 0), (good, -1), (good, 1 << 31), (good,), 5, (torch.zeros(3, 4, dtype=torch.int32), 0)):
        with pytest.raises(ValueError, match="solver_noise"):
            model.denoise(img, ids, txt, tids, y, ts, solver=prog, solver_noise=bad)
    with pytest.raises(ValueError, match="cache_threshold"):
        model.denoise(img, ids, txt, tids, y, ts, solver=prog, solver_noise=(good, 0), cache_threshold=0.1)
    assert model._engine is None, "a refused request created the engine"
    # a tensor of words (int32 bits or int64 values) is the list
    want = ([(0xffffffff, 2, 0, 0), (7, 2, 1, 0)], 3)
    assert model._check_solver_noise((torch.tensor([[-1, 2, 0, 0], [7, 2, 1, 0]], dtype=torch.int32), 3), prog, 2) == want
    assert model._check_solver_noise((torch.tensor([[0xffffffff, 2, 0, 0], [7, 2, 1, 0]], dtype=torch.int64), 3), prog, 2) == want


def test_chunked_batches_carry_the_ids():
    from fluxmi import solvers

    model = tiny_cpu_model()
    model.MAX_ENGINE_BATCH = 2
    whole, calls = model.denoise, []

    def single_pass(img, img_ids, txt, txt_ids, y, timesteps, **kw):
        if img.shape[0] > 2:
            return whole(img, img_ids, txt, txt_ids, y, timesteps, **kw)
        calls.append(dict(kw, img=img.clone()))
        return img + 1

    model.denoise = single_pass
    B, Li, Lt = 5, 4, 6
    img = torch.zeros(B, Li, 64) + torch.arange(B, dtype=torch.float32).reshape(B, 1, 1)  # sample b carries b
    ids, txt, tids, y = torch.zeros(B, Li, 3), torch.zeros(B, Lt, 128), torch.zeros(B, Lt, 3), torch.zeros(B, 64)
    ts = [1.0, 0.5, 0.0]
    prog = solvers.build_program("dpmpp_2m_sde", ts, 0.5)
    noise_ids = [st.ids_of(77, k) for k in range(B)]
    out = model.denoise(img, ids, txt, tids, y, ts, solver=prog, solver_noise=(noise_ids, 4))
    assert torch.equal(out, img + 1) and len(calls) == 3 and all(c["solver"] is prog for c in calls)
    # equal passes of 2: (0, 1), (2, 3), (4, 4 again): every pass's ids are its images', the padded tail copies the last image's
    assert [c["solver_noise"] for c in calls] == [([noise_ids[0], noise_ids[1]], 4), ([noise_ids[2], noise_ids[3]], 4), ([noise_ids[4], noise_ids[4]], 4)]
    assert all(int(c["img"][k, 0, 0]) == c["solver_noise"][0][k][2] for c in calls for k in range(2))


# ---- the interfaces ---------------------------------------------------------------------------------------------------------------------
def test_ctypes_table_has_the_noise_entries():
    from fluxmi import _lib

    for name in ("fluxmi_philox_normal", "fluxmi_solver_step_noise", "fluxmi_engine_set_solver_noise"):
        assert name in _lib.EXPORTS
    assert len(_lib.lib.fluxmi_solver_step_noise.argtypes) == len(_lib.lib.fluxmi_solver_step.argtypes) + 2  # + ids, eval_offset
    assert len(_lib.lib.fluxmi_philox_normal.argtypes) == 7 and len(_lib.lib.fluxmi_engine_set_solver_noise.argtypes) == 4
    assert _lib.lib.fluxmi_abi_version() == 5 and _lib.ABI_VERSION == 5
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "fluxmi.h")).read()
    assert all(f"int {n}(" in header for n in ("fluxmi_philox_normal", "fluxmi_solver_step_noise", "fluxmi_engine_set_solver_noise"))


def test_http_stochastic_fields():
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
    assert not any(k in seen for k in ("eta", "s_noise", "noise_seed", "sampler"))
    r = client.post("/generate", json={"prompt": "a", "sampler": "euler_ancestral", "eta": 0.5, "s_noise": 1.1, "noise_seed": (1 << 40) + 3})
    assert r.status_code == 200 and seen["sampler"] == "euler_ancestral" and seen["eta"] == 0.5 and seen["s_noise"] == 1.1
    assert seen["noise_seed"] == (1 << 40) + 3
    r = client.post("/generate", json={"prompt": "a", "sampler": "dpmpp_2m_sde", "eta": 0.0})
    assert r.status_code == 200 and seen["sampler"] == "dpmpp_2m_sde" and seen["eta"] == 0.0 and "s_noise" not in seen and "noise_seed" not in seen
    for bad in ({"sampler": "euler_a"}, {"eta": 1.5}, {"eta": -0.1}, {"s_noise": -1.0}, {"noise_seed": -1}, {"noise_seed": 1 << 64}):
        assert client.post("/generate", json=dict({"prompt": "a", "sampler": "euler_ancestral"}, **bad)).status_code == 422, bad
