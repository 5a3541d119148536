"""Live previews, progress and cancellation without a GPU: the fp32 emulation of the preview kernel against the fp64 definition
(tests/preview_ref.py), the factor fit and fold, generate's refusals, the exported symbols and the NDJSON stream of the HTTP endpoint."""
import base64
import io
import json
import os
import re
import threading

import numpy as np
import pytest
import torch

import preview_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the kernel's operation order against the definition ---------------------------------------------------------------------------
@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("grid,B", [((1, 1), 1), ((3, 2), 3), ((16, 16), 2)])
def test_fp32_emulation_against_fp64(grid, B, guided):
    """equal outside the band of half-integers the fp32 chain can cross, one level inside it, and the band is narrow for the reference alone"""
    x, pred, proj, t, s = pr.draws(B, grid, seed=11 + B, guided=guided, img_rows=grid[0] * grid[1] + 3, c_in=72)
    scale = s if guided else None
    want, y, delta = pr.reference_fp64(x, pred, t, proj, grid, scale)
    assert want.shape == (B, 2 * grid[0], 2 * grid[1], 3)
    share = float(pr.in_band(y, delta).mean())
    assert share <= 0.01, f"{share:.4f} of the reference's pixels lie inside the band: it could hide a failure"
    assert len(np.unique(want)) >= min(32, want.size // 2), "the inputs do not spread over the levels"
    got = pr.emulate_fp32(x, pred, t, proj, grid, scale)
    assert pr.check_band(got, want, y, delta, "fp32 emulation") == share


def test_clamps_and_nan():
    grid, B = (5, 7), 2
    x, pred, proj, t, s = pr.draws(B, grid, seed=3, amp=8.0)  # levels far outside 0..255 on both sides
    x[0, 4, 8:12] = np.nan                                      # channel 2 of token 4: its four pixels
    pred[1, 9, 63] = np.inf                                     # channel 15, sub-pixel 3 of token 9
    want, y, delta = pr.reference_fp64(x, pred, t, proj, grid)
    got = pr.emulate_fp32(x, pred, t, proj, grid)
    pr.check_band(got, want, y, delta, "clamped")
    assert (want == 0).mean() > 0.1 and (want == 255).mean() > 0.1
    ty, tx = divmod(4, 7)
    assert (got[0, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2] == 0).all(), "NaN maps to 0"
    ty, tx = divmod(9, 7)
    assert set(got[1, 2 * ty + 1, 2 * tx + 1].tolist()) <= {0, 255}


def test_the_layout_is_unpack():
    """slot-free check of the indexing: a preview whose factors pick latent channel c is FluxPipeline.unpack's channel c"""
    from flux_pipeline import FluxPipeline

    grid, B = (3, 5), 2
    x, pred, _, _, _ = pr.draws(B, grid, seed=5, amp=0.3)
    proj = np.zeros(51, np.float32)
    proj[3 * 6 + 0], proj[3 * 11 + 1], proj[3 * 0 + 2] = 1.0, 1.0, 1.0  # R = channel 6, G = channel 11, B = channel 0
    got, y, _ = pr.reference_fp64(x, pred, np.float32(0.0), proj, grid)
    lat = FluxPipeline.unpack(None, torch.from_numpy(x), 16 * grid[0], 16 * grid[1]).numpy()  # [B, 16, 2h, 2w]
    want = (0.5 * lat[:, [6, 11, 0]].astype(np.float64) + 0.5) * 255.0
    assert np.array_equal(y, want.transpose(0, 2, 3, 1))
    assert np.array_equal(got, pr.quantise(want.transpose(0, 2, 3, 1)))


# ---- 2. the factors ---------------------------------------------------------------------------------------------------------------------
def test_fit_recovers_a_linear_decoder():
    import util

    rng = np.random.default_rng(0)
    M, bias = rng.standard_normal((16, 3)), rng.standard_normal(3)
    z = rng.standard_normal((3, 16, 6, 5))
    rgb = np.einsum("nchw,ck->nkhw", z, M) + bias[None, :, None, None]
    m, b = util.fit_preview_factors(torch.from_numpy(z), torch.from_numpy(rgb))
    assert np.abs(np.asarray(m) - M).max() <= 1e-6 and np.abs(np.asarray(b) - bias).max() <= 1e-6
    with pytest.raises(ValueError, match="fit_preview_factors"):
        util.fit_preview_factors(torch.zeros(1, 4, 2, 2), torch.zeros(1, 3, 2, 2))


def test_scale_and_shift_fold():
    """bias' + M'^T z == bias + M^T (z / scale + shift) for the model's latent z"""
    import util
    from fluxmi import ops

    rng = np.random.default_rng(1)
    M, bias, z = rng.standard_normal((16, 3)), rng.standard_normal(3), rng.standard_normal(16)
    sf, sh = 0.3611, 0.1159
    p = np.asarray(util.fold_preview_factors(M.tolist(), bias.tolist(), sf, sh))
    assert p.shape == (51,)
    assert np.allclose(p[48:] + p[:48].reshape(16, 3).T @ z, bias + M.T @ (z / sf + sh), rtol=0, atol=1e-12)
    assert np.array_equal(np.asarray(util.fold_preview_factors(M.tolist(), bias.tolist(), 1.0, 0.0)), np.asarray(ops.preview_proj(M, bias)))
    with pytest.raises(ValueError, match="16"):
        util.fold_preview_factors(M[:15].tolist(), bias.tolist(), sf, sh)


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------
def test_generate_refusals():
    from flux_pipeline import FluxPipeline

    pipe = object.__new__(FluxPipeline)  # every check below precedes the first use of the pipeline's state
    with pytest.raises(ValueError, match="needs on_step"):
        pipe.generate("a", preview_every=2)
    for bad in (-1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="preview_every"):
            pipe.generate("a", preview_every=bad, on_step=lambda info: True)
    with pytest.raises(ValueError, match="callable"):
        pipe.generate("a", on_step=3)
    with pytest.raises(ValueError, match="preview_factors"):
        pipe.generate("a", on_step=lambda info: True, preview_factors=([[0.0] * 3] * 16, [0.0] * 3))


def test_generate_refused_under_a_process_group(monkeypatch):
    from flux_pipeline import FluxPipeline
    from fluxmi import dist as fdist

    monkeypatch.setattr(fdist, "world_size", lambda: 2)
    with pytest.raises(ValueError, match="process group"):
        object.__new__(FluxPipeline).generate("a", on_step=lambda info: True)


def test_denoise_argument_check():
    from modules.flux_model import Flux, PreviewCall

    ok = PreviewCall([0.0] * 51, (2, 2), 1, 0, 4, lambda *a: True)
    assert Flux._check_preview(None) is None and Flux._check_preview(ok).every == 1
    assert Flux._check_preview(ok._replace(every=0, proj=None)).proj is None
    for bad in (ok._replace(every=-1), ok._replace(eval_offset=-1), ok._replace(proj=[0.0] * 50), ok._replace(proj=[float("nan")] * 51),
                ok._replace(callback=None), ok._replace(grid=(2,))):
        with pytest.raises(ValueError, match="preview"):
            Flux._check_preview(bad)


# ---- 4. the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_abi():
    import fluxmi
    from fluxmi import _lib

    for name in ("fluxmi_latent_preview", "fluxmi_engine_set_preview", "fluxmi_engine_preview_stats"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
    assert _lib.lib.fluxmi_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "fluxmi.h")).read()
    assert int(re.search(r"#define FLUXMI_PREVIEW_DEPTH (\d+)", hdr).group(1)) == _lib.PREVIEW_DEPTH
    assert _lib.PREVIEW_SLOTS == _lib.PREVIEW_DEPTH + 1
    assert int(re.search(r"#define FLUXMI_CANCELLED (\d+)", hdr).group(1)) == _lib.CANCELLED
    e = fluxmi.GenerationCancelled(5, 12)
    assert isinstance(e, RuntimeError) and (e.evaluations, e.num_evaluations) == (5, 12)
    # host-side argument validation needs no GPU
    assert _lib.lib.fluxmi_engine_set_preview(None, None, 1, 1, 1, 0, 1, None, None) != 0
    assert _lib.lib.fluxmi_latent_preview(None, None, None, None, None, None, None, None, 1, 1, 1, 64, 64, 1, 1, None) != 0
    assert b"latent_preview" in _lib.lib.fluxmi_last_error()


# ---- 5. the HTTP stream --------------------------------------------------------------------------------------------------------------------
class FakePipeline:
    """generate() calls on_step for `n` evaluations (a preview at every preview_every-th), stops when it returns False"""

    def __init__(self, n=5):
        self.n, self.calls, self.answers, self.gate = n, [], [], None

    def generate(self, on_step=None, preview_every=0, **kwargs):
        from fluxmi import GenerationCancelled

        self.calls.append(dict(kwargs, preview_every=preview_every, on_step=on_step))
        for j in range(self.n if on_step is not None else 0):
            if self.gate is not None and j == 1:
                self.gate.wait(10)
            pv = np.full((1, 4, 6, 3), 40 * j, np.uint8) if preview_every and j % preview_every == 0 else None
            r = on_step({"evaluation": j, "num_evaluations": self.n, "step": j // 2, "preview": pv})
            self.answers.append(r)
            if r is False:
                raise GenerationCancelled(j + 1, self.n)
        if kwargs.get("prompt") == "boom":
            raise RuntimeError("no such thing")
        return io.BytesIO(b"\xff\xd8JPEG")


def test_ndjson_stream():
    from fastapi.testclient import TestClient
    from PIL import Image

    import api

    fake = FakePipeline()
    api.app.state.model = fake
    client = TestClient(api.app)
    r = client.post("/generate", json={"prompt": "a"})
    assert r.status_code == 200 and r.headers["content-type"] == "image/jpeg" and r.content == b"\xff\xd8JPEG"
    assert "on_step" not in {k for k, v in fake.calls[-1].items() if v is not None} and fake.calls[-1]["preview_every"] == 0
    assert "stream" not in fake.calls[-1]
    assert client.post("/generate", json={"prompt": "a", "preview_every": 2}).status_code == 422
    assert client.post("/generate", json={"prompt": "a", "stream": True, "preview_every": -1}).status_code == 422
    r = client.post("/generate", json={"prompt": "a", "stream": True, "preview_every": 2})
    assert r.status_code == 200 and r.headers["content-type"].startswith("application/x-ndjson")
    ev = [json.loads(line) for line in r.text.splitlines()]
    assert [e["event"] for e in ev] == ["progress"] * 5 + ["result"]
    assert [e["evaluation"] for e in ev[:5]] == list(range(5)) and all(e["num_evaluations"] == 5 for e in ev[:5])
    assert [e["step"] for e in ev[:5]] == [0, 0, 1, 1, 2]
    assert [e["preview"] is not None for e in ev[:5]] == [True, False, True, False, True]
    im = Image.open(io.BytesIO(base64.b64decode(ev[2]["preview"])))
    assert im.size == (6, 4) and abs(int(np.asarray(im).mean()) - 80) <= 2
    assert base64.b64decode(ev[5]["image"]) == b"\xff\xd8JPEG"
    assert fake.calls[-1]["preview_every"] == 2 and "stream" not in fake.calls[-1]
    # progress only
    ev = [json.loads(line) for line in client.post("/generate", json={"prompt": "a", "stream": True}).text.splitlines()]
    assert len(ev) == 6 and all(e["preview"] is None for e in ev[:5])
    # an error in the worker is the last line
    ev = [json.loads(line) for line in client.post("/generate", json={"prompt": "boom", "stream": True}).text.splitlines()]
    assert ev[-1] == {"event": "error", "message": "no such thing"} and len(ev) == 6


def test_a_closed_stream_cancels():
    """closing the response's iterator -- a client that went away -- makes the next on_step return False"""
    import api

    fake = FakePipeline(n=6)
    fake.gate = threading.Event()  # the worker waits in front of evaluation 1 until the stream is closed
    gen = api.stream_events(fake, {"prompt": "a"})
    first = json.loads(next(gen))
    assert first["event"] == "progress" and first["evaluation"] == 0
    gen.close()
    fake.gate.set()
    for t in threading.enumerate():
        if t.name == "fluxmi-stream":
            t.join(10)
    assert fake.answers == [True, False], "the on_step behind the close must cancel"
