"""The image resampler on the GPU (csrc/resample.hip): fluxmi.ops.resize_u8 against PIL.Image.resize, byte for byte, no tolerance and no
excluded pixel (compared with Pillow 12.2.0).  Input and output are windows of sentinel-filled frames (test_preprocess_gpu.Framed), once
4-byte aligned and once not; the frames must stay intact.  Then the pipeline: image_resize="native" gives the latents of "pil" bit for bit."""
import numpy as np
import pytest
import torch
from PIL import Image

from test_preprocess_gpu import Framed, ops, tiny_pipeline  # noqa: F401  (ops is a fixture)

pytestmark = pytest.mark.gpu

PIL_FILTERS = {"box": Image.BOX, "bilinear": Image.BILINEAR, "hamming": Image.HAMMING, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}
TB, TR, MID_ROWS = 256, 16, 128  # asserted against the exported constants below
# (H, W) -> (h, w); c = channels.  fused: what resample_plan must say (None: one axis only, no plan to check)
SHAPES = {
    "1x1_up": (lambda c: ((1, 1), (5, 7)), True),
    "to_1x1": (lambda c: ((7, 5), (1, 1)), True),
    "rows_kept_w_up": (lambda c: ((20, 31), (20, 47)), None),
    "cols_kept_h_down": (lambda c: ((37, 53), (11, 53)), None),
    "rows_kept_w_down": (lambda c: ((37, 53), (37, 20)), None),
    "cols_kept_h_up": (lambda c: ((20, 31), (47, 31)), None),
    "h_up_w_down": (lambda c: ((33, 45), (70, 19)), True),
    "tile_plus_1": (lambda c: ((40, 200), (TR + 1, TB // c + 1)), True),
    "tile_minus_1": (lambda c: ((40, 200), (TR - 1, TB // c - 1)), True),
    "just_fused": (lambda c: ((MID_ROWS, 4), (1, 3)), True),          # every input row under the one tile: exactly the LDS budget
    "just_two_launches": (lambda c: ((MID_ROWS + 1, 4), (1, 3)), False),  # one row more: the horizontal-only + vertical-only launches
}


def pil_resize(img: np.ndarray, size, filter: str) -> np.ndarray:
    return np.stack([np.asarray(Image.fromarray(x).resize(size, PIL_FILTERS[filter])) for x in img])


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("filter", list(PIL_FILTERS))
def test_resize_equals_pil(ops, dev, filter, C, shape):
    assert (ops.RESAMPLE_TILE_BYTES, ops.RESAMPLE_TILE_ROWS, ops.RESAMPLE_LDS_MID_BYTES // ops.RESAMPLE_TILE_BYTES) == (TB, TR, MID_ROWS)
    make, fused = SHAPES[shape]
    (H, W), (h, w) = make(C)
    if fused is not None:
        assert ops.resample_plan(2, H, W, C, h, w, filter) == (fused, 0 if fused else 2 * H * ((w * C + 3) // 4 * 4))
    rng = np.random.default_rng(H * 1000 + W)
    dims = (2, H, W, 3) if C == 3 else (2, H, W)
    for family in ("bytes", "0_255"):  # the second: the negative lobes overshoot and the clip works at both ends
        img = rng.integers(0, 256, dims, dtype=np.uint8) if family == "bytes" else (rng.integers(0, 2, dims) * 255).astype(np.uint8)
        want = pil_resize(img, (w, h), filter)
        for aligned in (True, False):
            src, out = Framed(dev, 2, H, W, C, aligned, img), Framed(dev, 2, h, w, C, aligned)
            got = ops.resize_u8(src.win, (w, h), filter, out=out.win)
            assert got.data_ptr() == out.win.data_ptr()
            assert np.array_equal(out.get(), want), (family, aligned, np.argwhere(out.get() != want)[:4])
            assert out.intact() and src.intact() and np.array_equal(src.get(), img), (family, aligned, "a frame or the input was written")
    if shape == "h_up_w_down":
        x = torch.from_numpy(img).to(dev)
        assert torch.equal(ops.resize_u8(x, (w, h), filter), ops.resize_u8(x, (w, h), filter)), "two runs differ"
        assert torch.equal(ops.resize_u8(x, (W, H), filter), x), "the image's own size copies it"


def test_pipeline_native_resize_gives_the_latents_of_pil(dev):
    import types

    import depth_ref as dr
    import preprocess_ref as pr
    from fluxmi import synth
    from modules.depth import DepthAnythingNative
    from modules.image_embedders import ReduxImageEncoder
    from modules.ip_adapter import clip_preprocess

    g = torch.Generator().manual_seed(1)
    prompt = {"txt": 0.1 * torch.randn(1, 32, 128, generator=g), "vec": torch.randn(1, 64, generator=g)}
    photo = pr.family("smooth", 91, 61, seed=9)
    kw = dict(width=64, height=96, num_steps=4, seed=7, silent=True, output_type="latent")
    pipe = tiny_pipeline(dev, control=True)
    requests = [dict(init_image=photo, strength=0.6, control_image=photo), dict(control_image=photo, control_preprocess="canny")]
    for req in requests:
        lat = {}
        for mode in ("pil", "native"):
            torch.manual_seed(5)  # the VAE encoder's Gaussian sample
            lat[mode] = pipe.generate(prompt, **kw, **req, image_resize=mode)
        assert torch.isfinite(lat["pil"]).all() and torch.equal(lat["native"], lat["pil"]), sorted(req)
    # the Kontext reference (snapped to a preferred size, LANCZOS) and the depth estimator's bicubic resize behind the LANCZOS one
    ref = {m: pipe.prepare_kontext_reference(photo, generator=torch.Generator().manual_seed(3), image_resize=m) for m in ("pil", "native")}
    assert torch.equal(ref["native"][0], ref["pil"][0]) and torch.equal(ref["native"][1], ref["pil"][1])
    cfg = dr.tiny_config()
    pipe.depth_model = DepthAnythingNative(cfg)
    pipe.depth_model.load_state_dict(synth.make_depth_anything_state_dict(cfg, 0), strict=True)
    pipe.depth_model = pipe.depth_model.to(device=dev, dtype=torch.bfloat16)
    dmap = {m: pipe.preprocess_control(photo, "depth_anything", 64, 96, depth_resolution=56, image_resize=m, on_device=m == "native")
            for m in ("pil", "native")}
    assert dmap["native"].is_cuda and not dmap["pil"].is_cuda and torch.equal(dmap["native"].cpu(), dmap["pil"])
    # SigLIP's and CLIP-vision's preprocessing: the pixel values a tower sees do not depend on who resized
    assert torch.equal(clip_preprocess(photo, 224, dev), clip_preprocess(photo, 224))
    siglip = types.SimpleNamespace(image_size=384)
    assert torch.equal(ReduxImageEncoder.preprocess(siglip, photo, dev), ReduxImageEncoder.preprocess(siglip, photo))
    assert np.array_equal(pipe.resize(photo, 64, 96).numpy(), np.asarray(Image.fromarray(photo).resize((64, 96), Image.LANCZOS)))
    with pytest.raises(ValueError, match="image_resize"):
        pipe.generate(prompt, **kw, control_image=photo, image_resize="bicubic")
