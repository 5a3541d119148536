"""FlowEdit without a GPU: the program tables (fluxmi/flowedit.py), the step split, the ids, the pipeline's refusals and the float64 reference
of the whole algorithm (tests/flowedit_ref.py) on a linear toy velocity, where two of the algorithm's properties can be checked exactly."""
import numpy as np
import pytest
import torch

import flowedit_ref as fr

TS = [1.0, 0.8125, 0.59375, 0.3125, 0.125, 0.0]


def test_build_program_rows():
    from fluxmi import flowedit

    for n_avg in (1, 3):
        p = flowedit.build_program(TS, n_avg)
        n = n_avg * (len(TS) - 1)
        assert len(p.coef) == len(p.ctl) == len(p.times) == len(p.step_of_eval) == n  # n_avg x coupled steps
        assert flowedit.needs_acc(p) == (n_avg > 1)
        for j in range(n):
            i, k = divmod(j, n_avg)
            w, dt, tn, om = p.coef[j]
            first, apply = p.ctl[j]
            assert (first, apply) == (int(k == 0), int(k == n_avg - 1))
            assert w == fr.f32(1.0 / n_avg) and dt == TS[i + 1] - TS[i]
            assert tn == (TS[i + 1] if apply else TS[i]) and om == 1.0 - tn
            assert p.times[j] == TS[i] and p.step_of_eval[j] == i
    assert flowedit.build_program([0.5], 2).coef == [] and flowedit.build_program([], 1).times == []
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="edit_n_avg"):
            flowedit.build_program(TS, bad)


def test_split_steps_edges():
    from fluxmi import flowedit

    T = 5
    assert flowedit.split_steps(T) == (0, T)                  # every step coupled
    assert flowedit.split_steps(T, None, 0) == (0, T)
    assert flowedit.split_steps(T, T, 0) == (0, T)
    assert flowedit.split_steps(T, 0, 0) == (T, T)            # nothing runs
    assert flowedit.split_steps(T, 3, 0) == (2, 5)            # steps 0, 1 skipped
    assert flowedit.split_steps(T, 3, 3) == (2, 2)            # n_min == n_max: no coupled step, the tail alone
    assert flowedit.split_steps(T, 5, 5) == (0, 0)
    assert flowedit.split_steps(T, 4, 1) == (1, 4)
    # the definition: step i is coupled iff n_min < T - i <= n_max
    for n_max in range(T + 1):
        for n_min in range(n_max + 1):
            a, b = flowedit.split_steps(T, n_max, n_min)
            assert [i for i in range(T) if n_min < T - i <= n_max] == list(range(a, b))
            assert [i for i in range(T) if T - i <= n_min] == list(range(b, T))
    for n_max, n_min in ((6, 0), (3, 4), (3, -1), (-1, -1), (2.0, 0), (3, True)):
        with pytest.raises(ValueError, match="edit_n_m"):
            flowedit.split_steps(T, n_max, n_min)


def test_edit_ids():
    from fluxmi import flowedit

    seed = (0xDEADBEEF << 32) | 0x12345678
    assert flowedit.edit_ids(seed, 3) == [(0x12345678, 0xDEADBEEF, 0, 1), (0x12345678, 0xDEADBEEF, 1, 1), (0x12345678, 0xDEADBEEF, 2, 1)]
    assert all(row[3] == 1 for row in flowedit.edit_ids(7, 4))  # column 3: never a stochastic sampler's draw (which uses 0)
    assert flowedit.edit_ids(7, 2, first_image=5)[1] == (7, 0, 6, 1)
    for bad in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            flowedit.edit_ids(bad, 1)


def test_abi_table_and_header():
    import os

    from fluxmi import _lib

    names = ("fluxmi_flowedit_couple", "fluxmi_flowedit_step", "fluxmi_engine_set_flow_edit", "fluxmi_engine_denoise_edit")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "fluxmi.h")).read()
    for name in names:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name) and f"int {name}(" in header
    assert len(_lib.lib.fluxmi_flowedit_couple.argtypes) == 13 and len(_lib.lib.fluxmi_flowedit_step.argtypes) == 16


# ---- the pipeline's refusals: every one a ValueError before any encoder or engine work ------------------------------------------------------
class _Untouchable:
    """a model / autoencoder / encoder that fails the test when anything but its channel counts is asked of it"""
    in_channels, out_channels = 64, 64

    def __getattr__(self, name):
        raise AssertionError(f"the refusal came too late: .{name} was touched")


def make_pipe(in_channels=64):
    from flux_pipeline import FluxPipeline

    pipe = FluxPipeline.__new__(FluxPipeline)
    pipe.name, pipe.debug, pipe.dtype, pipe.ae_dtype = "flux-dev", False, torch.bfloat16, torch.bfloat16
    pipe.device_flux = pipe.device_ae = pipe.device_clip = pipe.device_t5 = torch.device("cpu")
    model = _Untouchable()
    if in_channels != 64:
        model = type("M", (_Untouchable,), {"in_channels": in_channels, "out_channels": 64})()
    pipe.model, pipe.ae, pipe.clip, pipe.t5, pipe.redux, pipe.controlnet = model, _Untouchable(), _Untouchable(), _Untouchable(), None, None
    return pipe


PHOTO = np.zeros((64, 64, 3), dtype=np.uint8)
OK = dict(init_image=PHOTO, source_prompt="a photo of a cat", width=64, height=64, num_steps=8, seed=1, silent=True)


@pytest.mark.parametrize("kw, match", [
    (dict(init_image=None), "needs init_image"),
    (dict(strength=0.7), "strength 1.0"),
    (dict(sampler="heun"), "sampler"),
    (dict(negative_prompt="blurry", true_cfg_scale=2.0), "negative_prompt"),
    (dict(inpaint_mask=np.zeros((64, 64), dtype=np.uint8)), "inpaint_mask"),
    (dict(reference_image=PHOTO), "reference_image"),
    (dict(regions=[{"prompt": "a hat", "box": (0, 0, 1, 0.5)}]), "regions"),
    (dict(cache_threshold=0.1), "cache_threshold"),
    (dict(controlnet_image=PHOTO), "ControlNet"),
    (dict(controlnet_cond=torch.zeros(1, 16, 64)), "ControlNet"),
    (dict(ip_adapter_image=PHOTO), "IP-Adapter"),
    (dict(ip_adapter_image_embeds=torch.zeros(1, 768)), "IP-Adapter"),
    (dict(redux_image=PHOTO), "redux_image"),
    (dict(preview_every=2, on_step=lambda info: True), "preview_every"),
    (dict(edit_n_avg=0), "edit_n_avg"),
    (dict(edit_n_max=9), "edit_n_max"),
    (dict(edit_n_max=3, edit_n_min=4), "edit_n_min"),
    (dict(edit_n_min=-1), "edit_n_min"),
    (dict(num_images=17), "images"),
    (dict(noise_seed=-3), "noise_seed"),
])
def test_pipeline_refusals(kw, match):
    with pytest.raises(ValueError, match=match):
        make_pipe().generate("a photo of a dog", **{**OK, **kw})


def test_pipeline_refuses_conditioned_models_and_process_groups(monkeypatch):
    from fluxmi import dist as fdist

    for channels in (384, 128):  # Fill, Depth / Canny
        with pytest.raises(ValueError, match="Fill / Depth / Canny"):
            make_pipe(channels).generate("a photo of a dog", **OK)
    monkeypatch.setattr(fdist, "world_size", lambda: 2)
    with pytest.raises(ValueError, match="process group"):
        make_pipe().generate("a photo of a dog", **OK)


@pytest.mark.parametrize("kw", [dict(source_guidance=1.5), dict(edit_n_max=4), dict(edit_n_min=1), dict(edit_n_avg=2)])
def test_edit_arguments_need_a_source_prompt(kw):
    with pytest.raises(ValueError, match="need source_prompt"):
        make_pipe().generate("a photo of a dog", init_image=PHOTO, width=64, height=64, num_steps=8, seed=1, silent=True, **kw)


# ---- the float64 reference on a linear toy velocity  v(x, t, c) = A_c x + b_c ------------------------------------------------------------------
def toy(seed, same_A=True, same_all=False):
    g = torch.Generator().manual_seed(seed)
    D = 6
    A_src = 0.4 * torch.randn(D, D, generator=g, dtype=torch.float64)
    b_src = torch.randn(D, generator=g, dtype=torch.float64)
    A_tar = A_src if same_A or same_all else 0.4 * torch.randn(D, D, generator=g, dtype=torch.float64)
    b_tar = b_src if same_all else torch.randn(D, generator=g, dtype=torch.float64)
    x0 = torch.randn(5, D, generator=g, dtype=torch.float64)
    vel = lambda x, t, c: x @ (A_src if c == "src" else A_tar).T + (b_src if c == "src" else b_tar)
    return x0, vel


def test_fp64_identical_conditioning_returns_x0_exactly():
    """v_tar(zt) - v_src(zs) with zt = z + zs - x0 and z = x0 is v(zs) - v(zs) = 0 when zt == zs bit for bit: z = x0 gives zt = x0 + zs - x0,
    which float64 does not promise to be zs -- so the claim is checked on values where it is (dyadic x0 and draws: every sum is exact)"""
    x0, vel = toy(3, same_all=True)
    x0 = (x0 * 64).round() / 64
    g = torch.Generator().manual_seed(9)
    draws = [(torch.randn(x0.shape, generator=g, dtype=torch.float64) * 64).round() / 64 for _ in range(64)]
    ts = [1.0, 0.75, 0.5, 0.25, 0.0]  # dyadic times: (1 - t) x0 + t n is exact as well
    for n_avg in (1, 3):
        out = fr.edit_fp64(x0, vel, ts, n_avg=n_avg, normal=lambda k: draws[k])
        assert torch.equal(out, x0), f"n_avg {n_avg}: max |z - x0| = {(out - x0).abs().max().item():.3e}"
    # and on arbitrary values, to rounding
    x0b, velb = toy(4, same_all=True)
    out = fr.edit_fp64(x0b, velb, TS, n_avg=2)
    assert (out - x0b).abs().max().item() <= 1e-13


def test_fp64_noise_cancels_when_the_branches_share_A():
    """A_src = A_tar: v_tar(zt) - v_src(zs) = A (z - x0) + (b_tar - b_src) -- the draw cancels, so the result depends neither on the
    draws nor on n_avg beyond rounding, and differs from x0.  A wrong sign or a coupling that feeds the branches different noise breaks it."""
    x0, vel = toy(5, same_A=True)
    outs = []
    for n_avg, seed in ((1, 0), (3, 0), (1, 7), (4, 11)):
        g = torch.Generator().manual_seed(seed)
        outs.append(fr.edit_fp64(x0, vel, TS, n_avg=n_avg, normal=lambda k: torch.randn(x0.shape, generator=g, dtype=torch.float64)))
    scale = outs[0].abs().max().item()
    for o in outs[1:]:
        assert (o - outs[0]).abs().max().item() <= 1e-12 * max(1.0, scale)
    assert (outs[0] - x0).abs().max().item() > 1e-2
    # with different matrices the draws do matter (the test above is not vacuous)
    x0d, veld = toy(5, same_A=False)
    a = fr.edit_fp64(x0d, veld, TS, n_avg=1)
    g = torch.Generator().manual_seed(7)
    b = fr.edit_fp64(x0d, veld, TS, n_avg=1, normal=lambda k: torch.randn(x0d.shape, generator=g, dtype=torch.float64))
    assert (a - b).abs().max().item() > 1e-3


def test_fp64_split_skips_and_tail():
    """n_max < T starts later on the same schedule; n_min > 0 ends with an Euler tail on the target branch from zt of one more coupling"""
    x0, vel = toy(6, same_A=False)
    g = torch.Generator().manual_seed(2)
    draws = [torch.randn(x0.shape, generator=g, dtype=torch.float64) for _ in range(32)]
    nz = lambda k: draws[k]
    full = fr.edit_fp64(x0, vel, TS, normal=nz)
    assert torch.equal(fr.edit_fp64(x0, vel, TS, n_max=3, normal=nz), fr.edit_fp64(x0, vel, TS[2:], normal=nz))
    assert torch.equal(fr.edit_fp64(x0, vel, TS, n_max=0, normal=nz), x0)
    z3 = fr.edit_fp64(x0, vel, TS[:4], normal=nz)  # three coupled steps: draws 0, 1, 2
    t = TS[3]
    tail = z3 + ((1.0 - t) * x0 + t * draws[3]) - x0
    for a, b in zip(TS[3:-1], TS[4:]):
        tail = tail + (b - a) * vel(tail, a, "tar")
    got = fr.edit_fp64(x0, vel, TS, n_min=2, normal=nz)
    assert torch.equal(got, tail) and not torch.equal(got, full)
