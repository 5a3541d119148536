"""Control-map preprocessors on the GPU (csrc/preprocess.hip) against tests/preprocess_ref.py: Canny's classify map and its hysteresis byte
for byte, the luma against PIL, the blur against the rounded fp64 reference, and the pipeline's `control_preprocess`.  Operands are windows
of sentinel-filled buffers with a wider row stride, once 4-byte aligned (the kernels' dword path) and once not (their byte path); the frame
around every output must stay intact."""
import numpy as np
import pytest
import torch

import preprocess_ref as pr
from helper_refs import sentinel_like

pytestmark = pytest.mark.gpu

T = pr.TILE  # the classify tile and the hysteresis tile, height and width: all 32
SIZES = [(1, 1), (1, 7), (2, 3), (T - 1, T + 1), (T, T), (T + 1, T - 1), (2 * T + 3, 3 * T + 1)]
THRESHOLDS = [(0, 0), (100, 200), (200, 100), (150, 150), (2 * 1020, 2 * 1020 + 1)]


@pytest.fixture(scope="module")
def ops():
    from fluxmi import ops as o

    return o


class Framed:
    """a [B, H, W(, C)] uint8 window one row and a few bytes inside a sentinel-filled [B, H + 2, LD] buffer"""

    def __init__(self, dev, B, H, W, C=1, aligned=True, data=None):
        wb = W * C
        self.ld = (wb + 8 + 3) // 4 * 4 + (0 if aligned else 2)
        self.off = 4 if aligned else 3
        self.buf = sentinel_like((B, H + 2, self.ld // 2), dev).view(torch.uint8)
        self.rows, self.cols = slice(1, H + 1), slice(self.off, self.off + wb)
        win = self.buf[:, self.rows, self.cols]
        self.win = win.unflatten(-1, (W, C)) if C > 1 else win
        if data is not None:
            self.win.copy_(torch.as_tensor(data).reshape(self.win.shape).to(dev))

    def get(self) -> np.ndarray:
        return self.win.cpu().numpy()

    def intact(self) -> bool:
        full = self.buf.cpu().clone()
        clean = sentinel_like(tuple(full.view(torch.bfloat16).shape)).view(torch.uint8)
        full[:, self.rows, self.cols] = clean[:, self.rows, self.cols]
        return bool(torch.equal(full, clean))


def batch_of(fam, B, H, W, seed=0):
    return np.stack([pr.family(fam, H, W, seed + b) for b in range(B)])


# ---- classify --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", SIZES)
def test_classify_equals_the_definition(ops, dev, H, W, B):
    for k, fam in enumerate(pr.FAMILIES):
        img = batch_of(fam, B, H, W)
        for aligned in (True, False):
            src = Framed(dev, B, H, W, 3, aligned, img)
            for l2 in (False, True):
                for low, high in THRESHOLDS:
                    out = Framed(dev, B, H, W, 1, aligned)
                    got = ops.canny_classify(src.win, low, high, l2, out=out.win)
                    assert got.data_ptr() == out.win.data_ptr()
                    want = pr.canny_classify(img, low, high, l2)
                    assert np.array_equal(out.get(), want), (fam, aligned, l2, low, high, np.argwhere(out.get() != want)[:4])
                    assert out.intact(), (fam, aligned, l2, low, high, "the frame around the state map was written")
            assert src.intact() and np.array_equal(src.get(), img)
    dense = torch.from_numpy(batch_of("smooth", B, H, W)).to(dev)
    assert np.array_equal(ops.canny_classify(dense, 100, 200).cpu().numpy(), pr.canny_classify(dense.cpu().numpy(), 100, 200))


# ---- hysteresis alone, on synthetic state maps -----------------------------------------------------------------------------------------
def run_hysteresis(ops, dev, state, aligned=True):
    st = state if state.ndim == 3 else state[None]
    B, H, W = st.shape
    src = torch.from_numpy(st).to(dev)
    out = Framed(dev, B, H, W, 1, aligned)
    edges, rounds = ops.canny_hysteresis(src, out=out.win)
    assert edges.data_ptr() == out.win.data_ptr() and out.intact()
    assert np.array_equal(src.cpu().numpy(), st), "canny_hysteresis changed its input"
    got = out.get()
    assert np.array_equal(got, pr.hysteresis(st)), np.argwhere(got != pr.hysteresis(st))[:4]
    return got if state.ndim == 3 else got[0], rounds


@pytest.mark.parametrize("aligned", [True, False])
def test_hysteresis_serpentine_across_tiles(ops, dev, aligned):
    """a 1-pixel path crossing a 3 x 3 grid of tiles 24 times with ONE strong pixel at its start: every tile hands over to its neighbour many
    times, which only further rounds can do"""
    s = pr.serpentine(3 * T, 3 * T)
    got, rounds = run_hysteresis(ops, dev, s, aligned)
    assert np.array_equal(got, (s > 0) * 255) and rounds >= 2
    cut = pr.serpentine(3 * T, 3 * T, gap=(5, T + 3))
    got, rounds = run_hysteresis(ops, dev, cut, aligned)
    assert rounds >= 2 and got[:20].sum() == (cut[:20] > 0).sum() * 255 and got[20, T + 4:].all() and not got[20, :T + 3].any() and not got[24:].any()


def test_hysteresis_corners_borders_and_trivial_maps(ops, dev):
    H, W = 2 * T + 3, 3 * T + 1
    diag = np.zeros((H, W), dtype=np.uint8)
    diag[T - 1, T - 1] = 2  # the last pixel of tile (0, 0) ...
    for k in range(9):
        diag[T + k, T + k] = 1  # ... meets tile (1, 1) through its corner only
    diag[T - 1, 2 * T] = 2  # the first pixel of the last row of tile (0, 2) ...
    for k in range(7):
        diag[T + k, 2 * T - 1 - k] = 1  # ... meets tile (1, 1) through its other upper corner
    diag[T + 20, 5:9] = 1  # and a weak segment that nothing seeds
    got, rounds = run_hysteresis(ops, dev, diag)
    assert got[T + 8, T + 8] == 255 and got[T + 6, 2 * T - 7] == 255 and not got[T + 20].any() and rounds >= 2
    weak = np.ones((H, W), dtype=np.uint8)
    got, rounds = run_hysteresis(ops, dev, weak)
    assert not got.any() and rounds == 1, "all weak, no strong: nothing survives, and the first round already changes nothing"
    got, rounds = run_hysteresis(ops, dev, np.full((H, W), 2, dtype=np.uint8))
    assert (got == 255).all() and rounds == 1
    ring = np.zeros((H, W), dtype=np.uint8)
    ring[0, :] = ring[-1, :] = ring[:, 0] = ring[:, -1] = 1
    ring[H - 1, W - 1] = 2
    got, rounds = run_hysteresis(ops, dev, ring, aligned=False)
    assert np.array_equal(got, (ring > 0) * 255)
    # a batch of different maps in one call, and the small sizes
    run_hysteresis(ops, dev, np.stack([diag, ring, weak]))
    rng = np.random.default_rng(3)
    for h, w in SIZES:
        run_hysteresis(ops, dev, rng.choice(np.array([0, 1, 2], dtype=np.uint8), (3, h, w), p=[0.55, 0.4, 0.05]))


# ---- the whole detector ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_canny_equals_the_reference(ops, dev, H, W):
    alone = {}
    for fam in pr.FAMILIES:
        img = pr.family(fam, H, W)
        for aligned in (True, False):
            src, out = Framed(dev, 1, H, W, 3, aligned, img[None]), Framed(dev, 1, H, W, 1, aligned)
            ops.canny(src.win, 100, 200, out=out.win)
            assert out.intact() and np.array_equal(out.get()[0], pr.canny(img, 100, 200)), (fam, aligned)
        alone[fam] = out.get()[0]
        x = torch.from_numpy(img[None]).to(dev)
        assert np.array_equal(ops.canny(x, 40, 90, True).cpu().numpy()[0], pr.canny(img, 40, 90, True)), (fam, "l2")
        assert torch.equal(ops.canny(x, 100, 200), ops.canny(x, 100, 200)), "two runs differ"
    # a sample alone equals the same sample among different neighbours in a batch
    fams = list(pr.FAMILIES)
    for order in (fams[:3], fams[3:], fams[::-1][:3]):
        got = ops.canny(torch.from_numpy(np.stack([pr.family(f, H, W) for f in order])).to(dev), 100, 200).cpu().numpy()
        for k, f in enumerate(order):
            assert np.array_equal(got[k], alone[f]), (f, order)


def test_canny_photo_sized_image_and_rounds(ops, dev):
    """512 x 384: 16 x 12 tiles; the run-to-run and the reference check at a size where rounds overlap in earnest"""
    img = np.stack([pr.family("smooth", 384, 512, 5), pr.family("noise", 384, 512, 6)])
    x = torch.from_numpy(img).to(dev)
    a, rounds = ops.canny(x, 100, 200, return_rounds=True)
    assert rounds >= 1 and np.array_equal(a.cpu().numpy(), pr.canny(img, 100, 200))
    for _ in range(3):
        assert torch.equal(ops.canny(x, 100, 200), a)


# ---- luma ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_gray_equals_pil(ops, dev, B):
    from PIL import Image

    for H, W in SIZES + [(5, 1030)]:
        img = batch_of("noise", B, H, W, seed=4)
        want = np.stack([np.array(Image.fromarray(x).convert("L")) for x in img])
        for aligned in (True, False):
            src, out = Framed(dev, B, H, W, 3, aligned, img), Framed(dev, B, H, W, 1, aligned)
            ops.rgb_to_gray(src.win, out=out.win)
            assert np.array_equal(out.get(), want) and out.intact(), (H, W, aligned)
        assert np.array_equal(ops.rgb_to_gray(torch.from_numpy(img).to(dev)).cpu().numpy(), want)


# ---- blur ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.5, 2.0, 8.0])
@pytest.mark.parametrize("C", [1, 3])
def test_blur_equals_the_rounded_fp64_reference(ops, dev, sigma, C):
    for s, c, H, W, seed in pr.BLUR_CASES:
        if (s, c) != (sigma, C):
            continue
        img = pr.blur_input(C, H, W, seed, B=3)
        ref = pr.blur_f64(img, sigma)
        want, excused = np.clip(np.rint(ref), 0, 255).astype(np.int64), pr.blur_excused(ref)
        assert excused.mean() < 0.01
        for aligned in (True, False):
            src, out = Framed(dev, 3, H, W, C, aligned, img), Framed(dev, 3, H, W, C, aligned)
            ops.gaussian_blur(src.win if C > 1 else src.win[..., None], sigma, out=out.win if C > 1 else out.win[..., None])
            got = out.get().reshape(img.shape).astype(np.int64)
            bad = got != want
            assert out.intact() and not (bad & ~excused).any() and (np.abs(got - want) <= 1).all(), (H, W, aligned, int((bad & ~excused).sum()))
        one = torch.from_numpy(img[1:2]).to(dev)
        assert np.array_equal(ops.gaussian_blur(one, sigma).cpu().numpy()[0], got[1]), "a sample alone differs from the same sample in a batch"
    const = torch.full((2, 45, 300, C), 201, dtype=torch.uint8, device=dev)
    assert torch.equal(ops.gaussian_blur(const, sigma), const), "a constant image must stay exactly constant"
    if C == 1:
        assert torch.equal(ops.gaussian_blur(const[..., 0], sigma), const[..., 0]), "[B, H, W] counts as one channel"


def test_refusals_name_the_limit(ops, dev):
    x = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="adjacent"):
        ops.canny(x.permute(0, 2, 1, 3), 1, 2)
    with pytest.raises(ValueError, match=r"\[B, H, W, 3\]"):
        ops.rgb_to_gray(x[..., :2])
    with pytest.raises(TypeError, match="uint8"):
        ops.canny(x.float(), 1, 2)
    with pytest.raises(ValueError, match="does not match"):
        ops.canny(x, 1, 2, out=torch.zeros(1, 8, 9, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="radius"):
        ops.gaussian_blur(x, 22.0)
    with pytest.raises(ValueError, match="1 or 3 channels"):
        ops.gaussian_blur(torch.zeros(1, 8, 8, 2, dtype=torch.uint8, device=dev), 1.0)
    with pytest.raises(ValueError, match="must not be img"):
        ops.gaussian_blur(x, 1.0, out=x)


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------------
def tiny_pipeline(dev, control: bool):
    """the tiny Depth / Canny model of tests/test_fill_gpu.py (control) or the tiny text-to-image model of tests/test_controlnet_gpu.py, with
    the tiny VAE of both"""
    import util
    from flux_pipeline import FluxPipeline
    from fluxmi import synth
    from modules.autoencoder import AutoEncoder, AutoEncoderParams

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    p = cfg.params
    p.hidden_size, p.num_heads, p.depth, p.depth_single_blocks, p.context_in_dim, p.vec_in_dim = 256, 2, 2, 2, 128, 64
    if control:
        p.in_channels, p.out_channels = 128, 64
    cfg.text_enc_max_length = 32
    cfg.ae_device = str(dev)
    cfg.ae_params = AutoEncoderParams(resolution=32, in_channels=3, ch=32, out_ch=3, ch_mult=[1, 2, 2, 2], num_res_blocks=1, z_channels=16,
                                      scale_factor=0.3611, shift_factor=0.1159)
    torch.manual_seed(0)
    ae_sd = {k: v.clone() for k, v in AutoEncoder(cfg.ae_params).state_dict().items()}
    pipe = FluxPipeline.load_pipeline_from_config(cfg, state_dict=synth.make_state_dict(cfg.params, seed=0), ae_state_dict=ae_sd)
    if not control:
        pipe.controlnet = util.load_controlnet(cfg, device=dev, state_dict=synth.make_controlnet_state_dict(cfg.params, 2, 1, 3, seed=0))
    pipe.compile()
    return pipe


@pytest.mark.parametrize("control", [True, False], ids=["depth_canny_model", "controlnet"])
def test_pipeline_control_preprocess(dev, control):
    from PIL import Image

    pipe = tiny_pipeline(dev, control)
    g = torch.Generator().manual_seed(1)
    prompt = {"txt": 0.1 * torch.randn(1, 32, 128, generator=g), "vec": torch.randn(1, 64, generator=g)}
    photo = pr.family("smooth", 90, 60, seed=9)
    resized = np.array(Image.fromarray(photo).resize((64, 96), Image.LANCZOS))
    edges = pipe.preprocess_control(photo, "canny", 64, 96)
    assert edges.dtype == torch.uint8 and edges.device.type == "cpu" and tuple(edges.shape) == (96, 64, 3)
    want = pr.canny(resized, 100, 200)
    assert want.any() and np.array_equal(edges.numpy(), np.repeat(want[..., None], 3, -1))
    assert np.array_equal(pipe.preprocess_control(Image.fromarray(photo), "canny", 64, 96, canny_low=50, canny_high=200, canny_l2=True).numpy()[..., 0],
                          pr.canny(resized, 50, 200, True))
    assert np.array_equal(pipe.preprocess_control(photo, "gray", 64, 96).numpy()[..., 1], np.array(Image.fromarray(resized).convert("L")))
    assert np.array_equal(pipe.preprocess_control(photo, "canny").numpy()[..., 2], pr.canny(photo, 100, 200)), "no size given: the photo's own"
    ref = pr.blur_f64(resized, 2.0)
    blur = pipe.preprocess_control(photo, "blur", 64, 96, blur_sigma=2.0).numpy().astype(np.int64)
    assert not ((blur != np.rint(ref)) & ~pr.blur_excused(ref)).any()

    name = "control_image" if control else "controlnet_image"
    kw = dict(width=64, height=96, num_steps=4, seed=7, silent=True, output_type="latent", **({} if control else dict(control_mode=1)))

    def gen(**k):
        torch.manual_seed(5)  # the VAE encoder's Gaussian sample
        return pipe.generate(prompt, **kw, **k)

    from_map = gen(**{name: edges})
    assert torch.isfinite(from_map).all()
    assert torch.equal(gen(**{name: photo}, control_preprocess="canny"), from_map), "photo + control_preprocess differs from the map itself"
    assert torch.equal(gen(**{name: edges}, control_preprocess=None), from_map), "control_preprocess=None differs from no argument"
    assert not torch.equal(gen(**{name: photo}), from_map), "the photo itself conditions differently from its edge map"
    other = gen(**{name: photo}, control_preprocess="canny", canny_low=20, canny_high=60)
    assert torch.equal(other, gen(**{name: pipe.preprocess_control(photo, "canny", 64, 96, canny_low=20, canny_high=60)}))
