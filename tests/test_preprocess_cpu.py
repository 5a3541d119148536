"""Control-map preprocessors, the parts that need no GPU: the numpy reference of the Canny definition (tests/preprocess_ref.py) behaves as
include/fluxmi.h says, the luma formula is PIL's, the fp64 blur preserves a constant, and the pipeline and the HTTP API refuse bad
requests by name before any work."""
import io

import numpy as np
import pytest
import torch

import preprocess_ref as pr


def test_gray_formula_is_pil_convert_l():
    from PIL import Image

    rng = np.random.default_rng(0)
    for H, W in ((1, 1), (7, 13), (64, 33)):
        rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        assert np.array_equal(pr.gray(rgb), np.array(Image.fromarray(rgb).convert("L")))
    corners = np.array([[[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 1, 1], [254, 255, 254]]], dtype=np.uint8)
    assert np.array_equal(pr.gray(corners), np.array(Image.fromarray(corners).convert("L")))


def step_image(H, W, col, height):
    img = np.zeros((H, W, 3), dtype=np.uint8)
    img[:, col:] = height
    return img


def test_vertical_step_gives_one_edge_column_at_the_documented_position():
    """a step of height h between columns c - 1 and c: m = 4 h at both, the tie keeps the left one (m > left, m >= right)"""
    H, W, c = 12, 20, 9
    st = pr.canny_classify(step_image(H, W, c, 200), 100, 200)
    want = np.zeros((H, W), dtype=np.uint8)
    want[:, c - 1] = 2
    assert np.array_equal(st, want)
    assert np.array_equal(pr.canny(step_image(H, W, c, 200), 100, 200), want // 2 * 255)
    # m = 4 * 25 = 100 <= low: nothing, not even weak; 4 * 26 = 104: weak only, which hysteresis drops
    assert not pr.canny_classify(step_image(H, W, c, 25), 100, 200).any()
    weak = pr.canny_classify(step_image(H, W, c, 26), 100, 200)
    assert np.array_equal(weak, want // 2) and not pr.canny(step_image(H, W, c, 26), 100, 200).any()
    # the same step as rows: the upper row of the two is kept
    rows = np.zeros((H, W), dtype=np.uint8)
    rows[c - 1, :] = 2
    assert np.array_equal(pr.canny_classify(step_image(W, H, c, 200).transpose(1, 0, 2).copy(), 100, 200), rows)


def test_hysteresis_keeps_what_touches_a_strong_pixel():
    s = np.zeros((9, 12), dtype=np.uint8)
    s[2, 1:7] = 1          # a weak segment ...
    s[3, 7] = 2            # ... touching a strong pixel diagonally
    s[6, 2:6] = 1          # an isolated weak segment
    s[8, 11] = 2           # a lone strong pixel
    want = np.zeros_like(s)
    want[2, 1:7] = want[3, 7] = want[8, 11] = 255
    assert np.array_equal(pr.hysteresis(s), want)
    assert not pr.hysteresis(np.ones((5, 5), dtype=np.uint8)).any()
    assert (pr.hysteresis(np.full((5, 5), 2, dtype=np.uint8)) == 255).all()
    # the serpentine of the GPU test: whole with its seed, only the seeded part once it is cut
    T = pr.TILE
    full = pr.serpentine(3 * T, 3 * T)
    assert np.array_equal(pr.hysteresis(full), (full > 0) * 255)
    cut = pr.serpentine(3 * T, 3 * T, gap=(5, T + 3))
    got = pr.hysteresis(cut)
    assert got[0, 0] == 255 and got[:20].sum() == (cut[:20] > 0).sum() * 255 and not got[24:].any()
    assert got[20, T + 4:].all() and not got[20, :T + 3].any()  # row 20 runs right to left: the part behind the gap is lost


@pytest.mark.parametrize("fam", pr.FAMILIES)
def test_threshold_rules(fam):
    img = pr.family(fam, 40, 53, seed=2)
    assert np.array_equal(pr.canny_classify(img, 200, 100), pr.canny_classify(img, 100, 200)), "swapped thresholds are sorted"
    e = [pr.canny(img, low, 200) for low in (0, 40, 100, 200)]
    for a, b in zip(e[:-1], e[1:]):
        assert not (b & ~a).any(), "raising low added an edge"
    # low == high: no weak pixel survives non-maximum suppression as weak
    assert not (pr.canny_classify(img, 150, 150) == 1).any()
    assert not pr.canny_classify(img, 2 * 1020, 2 * 1020 + 5).any(), "no L1 magnitude exceeds 2 * 1020"


def test_l2_magnitude_against_squared_thresholds():
    """on an axis-aligned step dy = 0, so dx^2 against squared thresholds classifies exactly like |dx| against the plain ones; on noise the
    two norms differ"""
    img = step_image(10, 16, 5, 90)
    assert np.array_equal(pr.canny_classify(img, 100, 200, l2=True), pr.canny_classify(img, 100, 200))
    noise = pr.family("noise", 32, 32)
    dx, dy, m1 = pr.sobel(noise)
    _, _, m2 = pr.sobel(noise, l2=True)
    assert (m2 <= m1 * m1).all() and (2 * m2 >= m1 * m1).all()  # same channel or not, |.|_2^2 <= |.|_1^2 <= 2 |.|_2^2 holds for the maxima
    assert not np.array_equal(pr.canny_classify(noise, 300, 600, l2=True), pr.canny_classify(noise, 300, 600))


def test_tie_rule_and_channel_choice():
    eq = pr.family("equal", 24, 31)
    dx, dy, m = pr.sobel(eq)
    p = np.pad(eq[..., 0].astype(np.int64), 1, mode="edge")
    assert np.array_equal(dx, (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])), "equal channels: channel 0"
    ch = pr.family("channels", 48, 48)
    per = [pr.sobel(np.repeat(ch[..., c:c + 1], 3, -1))[2] for c in range(3)]
    assert np.array_equal(pr.sobel(ch)[2], np.maximum(np.maximum(per[0], per[1]), per[2]))
    assert len({int(np.argmax(np.stack(per)[:, y, x])) for y, x in ((5, 12), (24, 30), (40, 40))}) >= 2, "one channel wins everywhere"


@pytest.mark.parametrize("sigma", [0.5, 2.0, 8.0])
def test_blur_reference(sigma):
    w = pr.blur_taps(sigma)
    assert len(w) == 2 * int(np.ceil(3 * sigma)) + 1 and abs(w.sum() - 1.0) < 1e-15 and np.array_equal(w, w[::-1])
    const = np.full((9, 11, 3), 201, dtype=np.uint8)
    assert np.abs(pr.blur_f64(const, sigma) - 201.0).max() < 1e-11, "the fp64 blur of a constant image is that constant"
    img = pr.blur_input(3, 20, 30, 0)[0]
    b = pr.blur_f64(img, sigma)
    assert b.min() >= img.min() - 1e-9 and b.max() <= img.max() + 1e-9
    # the border is replicated: blurring an image padded by its own edge and cropping gives the same interior
    r = len(w) // 2
    padded = np.pad(img, ((r, r), (r, r), (0, 0)), mode="edge")
    assert np.abs(pr.blur_f64(padded, sigma)[r:-r, r:-r] - b).max() < 1e-9


def test_blur_cases_leave_under_one_percent_to_rounding():
    for sigma, C, H, W, seed in pr.BLUR_CASES:
        ref = pr.blur_f64(pr.blur_input(C, H, W, seed, B=3), sigma)
        assert pr.blur_excused(ref).mean() < 0.01, (sigma, C, H, W)


# ---- ops / pipeline / HTTP refusals ----------------------------------------------------------------------------------------------------
def test_ops_refuse_by_name():
    from fluxmi import ops

    assert ops.CANNY_TILE == pr.TILE
    with pytest.raises(RuntimeError, match="GPU"):
        ops.canny(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), 100, 200)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.rgb_to_gray(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    for bad in ((-1, 5), (1.5, 5), (True, 5), (5, 2 ** 31)):
        with pytest.raises(ValueError, match="expected an integer"):
            ops.canny_thresholds(*bad)
    assert (ops.blur_radius(0.5), ops.blur_radius(2), ops.blur_radius(8.0), ops.blur_radius(21.25)) == (2, 6, 24, 64)
    for bad in (0, -1.0, 21.4, float("nan"), float("inf"), "wide"):
        with pytest.raises(ValueError, match="radius"):
            ops.blur_radius(bad)


class _FakeModel:
    """stands in for Flux in FluxPipeline: records the denoise calls"""

    def __init__(self, params, extra=0):
        self.params, self.calls = params, []
        self.in_channels, self.out_channels = params.in_channels + extra, params.in_channels

    def denoise(self, img, img_ids, txt, txt_ids, y, timesteps, **kw):
        self.calls.append(dict(kw, ts=list(timesteps)))
        return img


def make_pipe(extra=0):
    import util
    from flux_pipeline import FluxPipeline

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    p = cfg.params
    p.hidden_size, p.num_heads, p.depth, p.depth_single_blocks, p.context_in_dim, p.vec_in_dim = 256, 2, 1, 1, 128, 64
    pipe = FluxPipeline.__new__(FluxPipeline)
    pipe.name, pipe.debug, pipe.dtype, pipe.ae_dtype = "flux-dev", False, torch.bfloat16, torch.bfloat16
    pipe.device_flux = pipe.device_ae = pipe.device_clip = pipe.device_t5 = torch.device("cpu")
    pipe.model, pipe.ae, pipe.clip, pipe.t5, pipe.rng = _FakeModel(p, extra), None, None, None, torch.Generator(device="cpu")
    pipe.redux, pipe.controlnet, pipe.config = None, None, cfg
    return pipe


def test_pipeline_refusals():
    g = torch.Generator().manual_seed(1)
    prompt = {"txt": 0.1 * torch.randn(1, 32, 128, generator=g), "vec": torch.randn(1, 64, generator=g)}
    KW = dict(width=64, height=64, num_steps=4, seed=7, silent=True, output_type="latent")
    photo = np.random.default_rng(0).integers(0, 256, (48, 40, 3), dtype=np.uint8)
    pipe = make_pipe(extra=64)
    assert pipe.conditioning_kind() == "control"
    with pytest.raises(ValueError, match="control_preprocess needs control_image"):
        pipe.generate(prompt, control_preprocess="canny", **KW)
    with pytest.raises(ValueError, match="img_cond / controlnet_cond"):
        pipe.generate(prompt, control_preprocess="canny", img_cond=torch.zeros(1, 16, 64), **KW)
    with pytest.raises(ValueError, match="img_cond / controlnet_cond"):
        make_pipe().generate(prompt, control_preprocess="gray", controlnet_cond=torch.zeros(1, 16, 64), **KW)
    with pytest.raises(ValueError, match="control_preprocess='depth'"):
        pipe.generate(prompt, control_image=photo, control_preprocess="depth", **KW)
    for bad in (dict(canny_low=-1), dict(canny_high=-5), dict(canny_low=99.5), dict(canny_high=True)):
        with pytest.raises(ValueError, match="canny_low=.* / canny_high=.*integers >= 0"):
            pipe.generate(prompt, control_image=photo, control_preprocess="canny", **bad, **KW)
    with pytest.raises(ValueError, match="canny_l2"):
        pipe.generate(prompt, control_image=photo, control_preprocess="canny", canny_l2=1, **KW)
    for bad in (0.0, -2.0, 21.5, float("nan")):
        with pytest.raises(ValueError, match="blur_sigma"):
            pipe.generate(prompt, control_image=photo, control_preprocess="blur", blur_sigma=bad, **KW)
    with pytest.raises(ValueError, match="belong to control_preprocess"):
        pipe.generate(prompt, control_image=photo, canny_low=50, **KW)
    # the refusals come before any work: nothing reached the model, and the model-kind refusals of today still speak first where they apply
    assert pipe.model.calls == []
    with pytest.raises(ValueError, match="need a FLUX.1 Fill or Depth / Canny model"):
        make_pipe().generate(prompt, control_image=photo, control_preprocess="canny", **KW)
    # preprocess_control itself: the same argument checks, then the kernels -- which refuse a host tensor (there is no CPU path)
    with pytest.raises(ValueError, match="control_preprocess='pose'"):
        pipe.preprocess_control(photo, "pose")
    with pytest.raises(ValueError, match="blur_sigma"):
        pipe.preprocess_control(photo, "blur", blur_sigma=30.0)
    with pytest.raises(RuntimeError, match="GPU"):
        pipe.preprocess_control(photo, "canny", 64, 64)
    # control_preprocess=None is today's request
    plain = make_pipe()
    plain.generate(prompt, **KW)
    plain.generate(prompt, control_preprocess=None, **KW)
    assert len(plain.model.calls) == 2 and plain.model.calls[0] == plain.model.calls[1]


def test_http_fields():
    from fastapi.testclient import TestClient

    import api

    calls = []

    class Stub:
        def generate(self, **kw):
            calls.append(kw)
            return io.BytesIO(b"\xff\xd8jpeg-bytes\xff\xd9")

    f = api.GenerateArgs.model_fields
    for k in ("control_preprocess", "canny_low", "canny_high", "canny_l2", "blur_sigma"):
        assert k in f and f[k].default is None
    api.app.state.model = Stub()
    c = TestClient(api.app)
    base = {"prompt": "a cat on a bench", "width": 512, "height": 512, "num_steps": 4, "seed": 7}
    assert c.post("/generate", json=base).status_code == 200
    assert set(calls[-1]) == {"prompt", "width", "height", "num_steps", "guidance", "seed", "strength", "init_image"}
    r = c.post("/generate", json={**base, "control_image": "photo.png", "control_preprocess": "canny", "canny_low": 50, "canny_high": 200})
    assert r.status_code == 200 and r.content.startswith(b"\xff\xd8")
    kw = calls[-1]
    assert (kw["control_image"], kw["control_preprocess"], kw["canny_low"], kw["canny_high"]) == ("photo.png", "canny", 50, 200)
    assert "canny_l2" not in kw and "blur_sigma" not in kw
    r = c.post("/generate", json={**base, "controlnet_image": "photo.png", "control_preprocess": "blur", "blur_sigma": 4.5, "canny_l2": True})
    assert r.status_code == 200 and calls[-1]["blur_sigma"] == 4.5 and calls[-1]["canny_l2"] is True and "canny_low" not in calls[-1]
    for bad in ({"control_preprocess": "depth"}, {"canny_low": -1}, {"canny_high": 1.5}, {"blur_sigma": 0}, {"blur_sigma": -1.0}):
        assert c.post("/generate", json={**base, **bad}).status_code == 422, bad
