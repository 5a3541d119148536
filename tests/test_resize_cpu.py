"""The image resampler without a GPU: the written definition (tests/resize_ref.py) against Pillow, the host's coefficient tables
(fluxmi_resample_coeffs) against the definition, and the refusals.  Compared with Pillow 12.2.0."""
import numpy as np
import pytest
import torch
from PIL import Image

import resize_ref as rr

PIL_FILTERS = {"box": Image.BOX, "bilinear": Image.BILINEAR, "hamming": Image.HAMMING, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}
# (H, W) -> (h, w): the degenerate ones, a kept axis each way, up and non-integer down, the identity
SIZE_PAIRS = [((1, 1), (5, 7)), ((7, 5), (1, 1)), ((37, 53), (37, 20)), ((20, 31), (47, 31)), ((33, 45), (70, 19)), ((64, 48), (23, 100)),
              ((24, 18), (24, 18))]
AXES = [(1, 5), (7, 1), (20, 47), (53, 20), (37, 37), (300, 77), (129, 1)]  # in = 1, out = 1, an upscale, non-integer downscales, an identity


@pytest.mark.parametrize("filter", list(PIL_FILTERS))
def test_the_definition_equals_pil(filter):
    rng = np.random.default_rng(0)
    for (H, W), (h, w) in SIZE_PAIRS:
        for dims in ((H, W), (H, W, 3)):
            for img in (rng.integers(0, 256, dims, dtype=np.uint8), (rng.integers(0, 2, dims) * 255).astype(np.uint8)):
                want = np.asarray(Image.fromarray(img).resize((w, h), PIL_FILTERS[filter]))
                assert np.array_equal(rr.resize(img, (w, h), filter), want), ((H, W), (h, w), dims)


@pytest.mark.parametrize("filter", list(PIL_FILTERS))
def test_host_coefficients_equal_the_definition(filter):
    from fluxmi import ops

    for n_in, n_out in AXES:
        bounds, kk = ops.resample_coeffs(n_in, n_out, filter)
        want_bounds, want_kk = rr.coeffs(n_in, n_out, filter)
        assert np.array_equal(bounds.numpy(), want_bounds) and np.array_equal(kk.numpy(), want_kk), (n_in, n_out)
        assert (kk.sum(1) - (1 << rr.PRECISION_BITS)).abs().max() <= kk.shape[1], "a row of taps sums to 2^22 up to its roundings"


def test_refusals_name_what_is_not_provided():
    from flux_pipeline import IMAGE_RESIZERS, FluxPipeline
    from fluxmi import ops
    import util

    with pytest.raises(ValueError, match="4-channel"):
        ops.resize_u8(torch.zeros(1, 8, 8, 4, dtype=torch.uint8), (4, 4))
    for bad in ("nearest", "cubic", 3):
        with pytest.raises(ValueError, match="filter="):
            ops.resize_u8(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (4, 4), filter=bad)
    with pytest.raises(ValueError, match="width and height"):
        ops.resize_u8(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (4, 0))
    with pytest.raises(RuntimeError, match="not provided"):
        ops.resample_plan(1, 8, 100000, 3, 8, 1, "lanczos")  # one input row of a tile beyond the LDS stage
    assert IMAGE_RESIZERS == ("pil", "native") and util.ModelSpec.model_fields["image_resize"].default == "pil"
    p = object.__new__(FluxPipeline)
    p.upscaler, p.ae = None, object()
    with pytest.raises(ValueError, match="image_resize='bicubic'"):
        p.generate("a prompt", image_resize="bicubic")
    p.config = type("Cfg", (), {"image_resize": "native", "jpeg_encoder": "pil"})()
    assert p._image_resize(None) == "native" and p._image_resize("pil") == "pil"
