"""Tiled generation without a GPU: where the windows sit and how they are weighted (fluxmi/windows.py), the torch restatement of the update
(tests/window_ref.py) on the one case that has a closed form, the pipeline's refusals and the request schema."""
import math

import numpy as np
import pytest
import torch

import window_ref as wr
from test_flowedit_cpu import make_pipe


# ---- placement ----------------------------------------------------------------------------------------------------------------------------
def test_window_positions():
    from fluxmi.windows import window_positions

    assert window_positions(10, 4, 4) == [0, 4, 6]  # the last window snaps to the edge: an irregular overlap
    assert window_positions(10, 4, 3) == [0, 3, 6]
    assert window_positions(10, 10, 3) == [0]
    assert window_positions(10, 4, 6) == [0, 6]
    assert window_positions(10, 4, 100) == [0, 6]
    pos = window_positions(10, 4, 1)
    assert pos == list(range(7))
    cover = [sum(p <= i < p + 4 for p in pos) for i in range(10)]
    assert cover == [1, 2, 3, 4, 4, 4, 4, 3, 2, 1] and all(3 <= c <= 4 for c in cover[2:8])
    for canvas, window, stride in ((10, 4, 4), (10, 4, 3), (37, 8, 5), (64, 64, 48), (256, 64, 48), (7, 1, 1)):
        pos = window_positions(canvas, window, stride)
        assert pos[0] == 0 and pos[-1] == canvas - window and pos == sorted(pos)
        assert len(pos) == math.ceil((canvas - window) / stride) + 1
        assert all(any(p <= i < p + window for p in pos) for i in range(canvas))
    for bad in ((10, 11, 1), (10, 0, 1), (10, 4, 0), (10, 4, -1)):
        with pytest.raises(ValueError, match="windows"):
            window_positions(*bad)


# ---- weights ------------------------------------------------------------------------------------------------------------------------------
CASES = [(10, 4, 4), (10, 4, 3), (10, 4, 1), (10, 10, 1), (37, 8, 5), (128, 64, 48), (40, 32, 1)]


@pytest.mark.parametrize("profile", ["cosine", "uniform"])
@pytest.mark.parametrize("canvas, window, stride", CASES)
def test_window_weights(canvas, window, stride, profile):
    from fluxmi.windows import window_positions, window_weights

    pos = window_positions(canvas, window, stride)
    W = window_weights(canvas, window, pos, profile)
    assert W.dtype == torch.float32 and tuple(W.shape) == (len(pos), canvas) and torch.isfinite(W).all()
    inside = torch.zeros(len(pos), canvas, dtype=torch.bool)
    for k, p in enumerate(pos):
        inside[k, p:p + window] = True
    assert (W[~inside] == 0).all(), "a weight outside its window"
    assert (W[inside] > 0).all(), "a zero weight inside a window (the cosine profile is sampled at the half positions: > 0 everywhere)"
    n_cover = inside.sum(0)
    assert int(n_cover.max()) <= 32
    # every column sums to 1: at most 32 casts, each off by at most 2^-24 of a value <= 1
    err = (W.double().sum(0) - 1.0).abs().max().item()
    assert err <= 2.0 ** -22, f"column sums off by {err:.3e}"
    single = n_cover == 1
    assert (W[:, single].sum(0) == 1.0).all() and ((W[:, single] == 1.0) | (W[:, single] == 0.0)).all(), "one covering window must weigh exactly 1.0f"
    if profile == "uniform":
        want = inside.double() / n_cover.double()
        assert torch.equal(W, want.float())
    else:  # the definition, in double
        prof = torch.tensor([0.5 - 0.5 * math.cos(2.0 * math.pi * (i + 0.5) / window) for i in range(window)], dtype=torch.float64)
        raw = torch.zeros(len(pos), canvas, dtype=torch.float64)
        for k, p in enumerate(pos):
            raw[k, p:p + window] = prof
        assert torch.equal(W, (raw / raw.sum(0)).float())


def test_window_weights_refusals():
    from fluxmi.windows import plan, window_weights

    with pytest.raises(ValueError, match="profile"):
        window_weights(10, 4, [0, 6], "gaussian")
    with pytest.raises(ValueError, match="leave the canvas"):
        window_weights(10, 4, [0, 7])
    with pytest.raises(ValueError, match="under no window"):
        window_weights(10, 4, [0, 6])
    p = plan(6, 10, 4, 4, 2, 4)
    assert (p.row0, p.col0, p.ny, p.nx) == ([0, 2], [0, 4, 6], 2, 3) and tuple(p.Ny.shape) == (2, 6) and tuple(p.Nx.shape) == (3, 10)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def test_ref_one_window_is_the_euler_step():
    from fluxmi.windows import plan

    g = torch.Generator().manual_seed(3)
    N, h, w, C = 2, 4, 5, 16
    x = torch.randn(N, h, w, C, generator=g).bfloat16()
    v = torch.randn(N, h * w, C, generator=g).bfloat16()
    dt = -0.1875 + 2.0 ** -12  # no bf16 value: the product rounds
    dtf = torch.tensor(dt, dtype=torch.float32)
    for profile in ("cosine", "uniform"):
        p = plan(h, w, h, w, 1, 1, profile)
        assert p.row0 == [0] and p.col0 == [0] and (p.Ny == 1).all() and (p.Nx == 1).all()
        got, stream = wr.step(x, v, dt, p.row0, p.col0, p.Ny, p.Nx, h, w)
        want = (x.float() + (dtf * v.float().reshape(N, h, w, C)).bfloat16().float()).bfloat16()
        assert got.dtype == torch.bfloat16 and torch.equal(got, want)
        assert torch.equal(stream, got.reshape(N, h * w, C))
        # guided: x + dt * (u + s * (c - u)) on bf16 tensors
        u = torch.randn(N, h * w, C, generator=g).bfloat16()
        s = torch.tensor(3.5, dtype=torch.float32)
        gv = (u.float() + (s * (v.float() - u.float()).bfloat16().float()).bfloat16().float()).bfloat16().float()
        got2, stream2 = wr.step(x, torch.cat((v, u), 0), dt, p.row0, p.col0, p.Ny, p.Nx, h, w, scale=3.5)
        want2 = (x.float() + (dtf * gv.reshape(N, h, w, C)).bfloat16().float()).bfloat16()
        assert torch.equal(got2, want2) and torch.equal(stream2[:N], stream2[N:]) and torch.equal(stream2[:N], got2.reshape(N, h * w, C))


def test_ref_gather_and_blend():
    from fluxmi.windows import plan

    g = torch.Generator().manual_seed(4)
    N, C = 2, 8
    p = plan(6, 10, 4, 4, 2, 4, "cosine")
    x = torch.randn(N, 6, 10, C, generator=g).bfloat16()
    s = wr.gather(x, p.row0, p.col0, 4, 4)
    assert tuple(s.shape) == (N * 6, 16, C)
    assert torch.equal(s[(1 * 2 + 1) * 3 + 2].reshape(4, 4, C), x[1, 2:6, 6:10])
    # windows that all predict the same field blend to that field (weights sum to 1), up to the fp32 sum's rounding and one bf16 rounding
    field = torch.randn(N, 6, 10, C, generator=g).bfloat16()
    pred = wr.gather(field, p.row0, p.col0, 4, 4)
    got, _ = wr.step(torch.zeros_like(x), pred, 1.0, p.row0, p.col0, p.Ny, p.Nx, 4, 4)
    assert (got.float() - field.float()).abs().max().item() <= 2.0 ** -8 * field.float().abs().max().item()


# ---- the pipeline's refusals: every one a ValueError before any encoder or engine work ------------------------------------------------------
PHOTO = np.zeros((64, 64, 3), dtype=np.uint8)
OK = dict(width=160, height=96, tile_size=64, num_steps=8, seed=1, silent=True, output_type="latent")


@pytest.mark.parametrize("kw, match", [
    (dict(sampler="heun"), "tile_size.*sampler"),
    (dict(sampler="euler_ancestral"), "tile_size.*sampler"),
    (dict(negative_prompt="blurry", true_cfg_scale=2.0, guidance_rescale=0.5), "tile_size.*guidance shaping"),
    (dict(negative_prompt="blurry", true_cfg_scale=2.0, guidance_mode="apg"), "tile_size.*guidance shaping"),
    (dict(negative_prompt="blurry", true_cfg_scale=2.0, zero_init_steps=1), "tile_size.*guidance shaping"),
    (dict(init_image=PHOTO, inpaint_mask=np.zeros((64, 64), dtype=np.uint8)), "tile_size.*inpaint_mask"),
    (dict(reference_image=PHOTO), "tile_size.*reference_image"),
    (dict(mask_image=PHOTO), "tile_size.*Fill"),
    (dict(control_image=PHOTO), "tile_size.*Depth / Canny"),
    (dict(redux_image=PHOTO), "tile_size.*redux_image"),
    (dict(regions=[{"prompt": "a hat", "box": (0, 0, 1, 0.5)}]), "tile_size.*regions"),
    (dict(cache_threshold=0.1), "tile_size.*cache_threshold"),
    (dict(controlnet_image=PHOTO), "tile_size.*ControlNet"),
    (dict(controlnet_cond=torch.zeros(1, 60, 64)), "tile_size.*ControlNet"),
    (dict(ip_adapter_image=PHOTO), "tile_size.*IP-Adapter"),
    (dict(ip_adapter_image_embeds=torch.zeros(1, 768)), "tile_size.*IP-Adapter"),
    (dict(init_image=PHOTO, source_prompt="a photo of a cat"), "tile_size.*source_prompt"),
    (dict(preview_every=2, on_step=lambda info: True), "tile_size.*preview_every"),
    (dict(tile_overlap=0, num_images=6), "tile_size.*one engine pass"),                                     # 6 x 2 x 3 = 36 > 32
    (dict(tile_overlap=0, num_images=3, negative_prompt="blurry", true_cfg_scale=2.0), "tile_size.*one engine pass"),  # 2 x 18 > 32
    (dict(tile_size=48, tile_overlap=32, width=256, height=256), "tile_size.*one engine pass"),            # 14 x 14 windows
    (dict(tile_size=72), "tile_size"),
    (dict(tile_size=0), "tile_size"),
    (dict(tile_size=(64, 176)), "tile_size"),
    (dict(tile_size=(64, 64, 64)), "tile_size"),
    (dict(tile_size="64"), "tile_size"),
    (dict(tile_overlap=64), "tile_overlap"),
    (dict(tile_overlap=24), "tile_overlap"),
    (dict(tile_overlap=-16), "tile_overlap"),
    (dict(tile_weight="gaussian"), "tile_weight"),
    (dict(true_cfg_scale=2.0), "negative_prompt"),
])
def test_pipeline_refusals(kw, match):
    with pytest.raises(ValueError, match=match):
        make_pipe().generate("a wide valley", **{**OK, **kw})


def test_pipeline_refuses_conditioned_models_process_groups_and_a_canvas_the_vae_cannot_take(monkeypatch):
    from fluxmi import dist as fdist

    for channels in (384, 128):  # Fill, Depth / Canny
        with pytest.raises(ValueError, match="tile_size.*Fill / Depth / Canny"):
            make_pipe(channels).generate("a wide valley", **OK)
    # 2048 x 2048: 65536 latent pixels, a [P, P] score matrix of 8 GiB behind a 32-bit descriptor
    big = dict(OK, width=2048, height=2048, tile_size=1024, tile_overlap=0)
    with pytest.raises(ValueError, match="tile_size.*VAE"):
        make_pipe().generate("a wide valley", **{**big, "output_type": "jpeg"})
    with pytest.raises(ValueError, match="tile_size.*VAE"):
        make_pipe().generate("a wide valley", **{**big, "init_image": PHOTO, "strength": 0.5})
    monkeypatch.setattr(fdist, "world_size", lambda: 2)
    with pytest.raises(ValueError, match="tile_size.*process group"):
        make_pipe().generate("a wide valley", **OK)


@pytest.mark.parametrize("kw", [dict(tile_overlap=16), dict(tile_weight="uniform")])
def test_tile_arguments_need_a_tile_size(kw):
    with pytest.raises(ValueError, match="need tile_size"):
        make_pipe().generate("a wide valley", width=64, height=64, num_steps=8, seed=1, silent=True, **kw)


def test_check_tiles_plans():
    """what _check_tiles hands on: None for today's request, else the plan in tokens"""
    pipe = make_pipe()
    base = dict(sampler="euler", eta=1.0, s_noise=1.0, noise_seed=None, guidance_mode="cfg", guidance_rescale=0.0, zero_init_steps=0, apg_eta=1.0,
                apg_norm_threshold=0.0, apg_momentum=0.0, inpaint_mask=None, reference_image=None, redux_image=None, regions=None,
                source_prompt=None, mask_image=None, control_image=None, img_cond=None, inpaint_differential=False, controlnet_image=None,
                controlnet_cond=None, ip_adapter_image=None, ip_adapter_image_embeds=None, negative_ip_adapter_image=None, cache_threshold=0.0,
                preview_every=0, preview_factors=None, on_step=None, sigma_schedule=None, negative_prompt=None, true_cfg_scale=1.0,
                true_cfg_interval=(0.0, 1.0), num_images=1, prompt="p", output_type="latent", init_image=None, width=160, height=96,
                tile_size=None, tile_overlap=None, tile_weight="cosine")
    assert pipe._check_tiles(base) is None
    assert pipe._check_tiles(dict(base, width=64, height=64, tile_size=64)) is None           # one tile of the request's size: today's request
    assert pipe._check_tiles(dict(base, width=70, height=79, tile_size=(64, 64))) is None      # ... after the request's rounding to 16
    one = pipe._check_tiles(dict(base, width=64, height=64, tile_size=64, tile_weight="uniform"))
    assert (one.row0, one.col0) == ([0], [0]) and (one.Ny == 1).all() and (one.Nx == 1).all()
    p = pipe._check_tiles(dict(base, tile_size=64))                                              # default overlap: 64 // 4 = 16 px = 1 token
    assert (p.Hc, p.Wc, p.h, p.w, p.row0, p.col0) == (6, 10, 4, 4, [0, 2], [0, 3, 6])
    p = pipe._check_tiles(dict(base, tile_size=(64, 96), tile_overlap=32))
    assert (p.h, p.w, p.row0, p.col0) == (4, 6, [0, 2], [0, 4])
    p = pipe._check_tiles(dict(base, tile_size=48, tile_overlap=0))                              # 48 // 4 = 12 -> 0; explicit 0 too
    assert (p.h, p.w, p.row0, p.col0) == (3, 3, [0, 3], [0, 3, 6, 7])
    assert pipe._check_tiles(dict(base, tile_size=48)).col0 == [0, 3, 6, 7]


# ---- the HTTP schema ------------------------------------------------------------------------------------------------------------------------
def test_generate_schema_has_the_tile_fields():
    import api

    fields = api.GenerateArgs.model_fields
    for name in ("tile_size", "tile_overlap", "tile_weight"):
        assert name in fields and fields[name].default is None
    a = api.GenerateArgs(prompt="p", tile_size=[64, 96], tile_overlap=16, tile_weight="uniform")
    assert tuple(a.tile_size) == (64, 96) and a.tile_overlap == 16 and a.tile_weight == "uniform"
    assert api.GenerateArgs(prompt="p", tile_size=512).tile_size == 512
    with pytest.raises(Exception):
        api.GenerateArgs(prompt="p", tile_overlap=-16)
    props = api.GenerateArgs.model_json_schema()["properties"]
    assert {"tile_size", "tile_overlap", "tile_weight"} <= set(props)


def test_abi_table_and_header():
    import os

    from fluxmi import _lib

    names = ("fluxmi_window_gather", "fluxmi_window_step", "fluxmi_engine_set_windows", "fluxmi_engine_denoise_windows")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "fluxmi.h")).read()
    for name in names:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name) and f"int {name}(" in header
    assert len(_lib.lib.fluxmi_window_gather.argtypes) == 14 and len(_lib.lib.fluxmi_window_step.argtypes) == 19
    assert len(_lib.lib.fluxmi_engine_set_windows.argtypes) == 13 and len(_lib.lib.fluxmi_engine_denoise_windows.argtypes) == 12
