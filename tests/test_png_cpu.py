"""The PNG encoder's host side without a GPU: the plan and workspace arithmetic, the strip rule against tests/png_ref.py, the container
around a zlib payload, the refusals of the C entry points, and the pipeline's and the HTTP layer's output_type="png"."""
import ctypes as C
import io
import zlib

import numpy as np
import pytest

import png_ref as pr

SHAPES = [(1, 1, 1, 1), (1, 1, 7, 3), (1, 5, 1, 1), (1, 17, 33, 3), (1, 33, 259, 3), (1, 48, 1366, 3), (2, 9, 20, 3), (1, 2, 23300, 3),
          (1, 1024, 1024, 3), (1, 4096, 4096, 3)]


@pytest.mark.parametrize("B,H,W,Ch", SHAPES)
def test_plan_and_strip_rule(B, H, W, Ch):
    from fluxmi import ops

    assert (ops.PNG_STRIP_TARGET, ops.PNG_STRIP_ROWS, ops.PNG_FRAME_BYTES) == (pr.STRIP_TARGET, pr.STRIP_ROWS, pr.FRAME_BYTES)
    code, rows = ops.png_params(B, H, W, Ch, "paeth")
    assert code == 4 and rows == pr.strip_rows(W, Ch) and ops.png_strip_bound(70000) == pr.strip_bound(70000) == 70015
    assert rows == {1366: 16, 1024: 16, 4096: 5, 23300: 1}.get(W, rows)   # 16 rows of 4099 bytes: a strip beyond one stored block
    work, cap = ops.png_workspace_bytes(B, H, W, Ch)
    strips = pr.strips(B * H, W, Ch)
    slot = pr.strip_bound(rows * (1 + W * Ch))
    assert cap == pr.file_bound(B * H, W, Ch) and work % 16 == 0
    spill = 0 if rows * (1 + W * Ch) <= pr.STRIP_TARGET else len(strips) * (1 + W * Ch)   # a row beyond the target lives in `work`
    assert len(strips) * (slot + 20) + spill <= work <= len(strips) * (slot + 20 + 16 + 16) + spill + 5 * 256


def test_container_around_a_zlib_payload():
    from fluxmi import _lib, ops

    px = np.random.default_rng(0).integers(0, 256, (2, 9, 20, 3), dtype=np.uint8)
    z = zlib.compress(pr.filtered(px).tobytes(), 1)
    assert z[:2] == b"\x78\x01"
    buf, n = C.create_string_buffer(64), C.c_longlong(0)
    _lib.call("fluxmi_png_header", 2, 9, 20, 3, buf, 64, C.byref(n))
    assert n.value == 43 and buf.raw[:8] == b"\x89PNG\r\n\x1a\n" and buf.raw[41:43] == z[:2]
    head = bytearray(buf.raw[:41])
    head[33:37] = len(z).to_bytes(4, "big")   # the device writes the IDAT's length
    data = bytearray(bytes(head) + z + bytes(4) + b"\0\0\0\0IEND\xaeB`\x82")
    assert len(data) == pr.FRAME_BYTES - 6 + len(z) and ops.png_seal(data) >= 0.0
    assert int.from_bytes(data[-16:-12], "big") == zlib.crc32(bytes(data[37:-16]))
    from PIL import Image

    im = Image.open(io.BytesIO(bytes(data)))
    im.load()
    assert np.array_equal(np.asarray(im), px.reshape(18, 20, 3))
    with pytest.raises(RuntimeError, match="png_seal"):
        ops.png_seal(bytearray(data[:-1]))


@pytest.mark.parametrize("kw, match", [
    (dict(C=2), "C=2"), (dict(C=4), "C=4"), (dict(W=0), "W=0"), (dict(H=-1), "H=-1"), (dict(B=3, H=2 ** 30), "2\\^31"),
    (dict(W=2 ** 29, H=1), "2\\^30"), (dict(H=70000, W=40000), "IDAT"), (dict(H=300000000, W=1, C=1, ld=1), "18750000 strips"), (dict(filter=6), "filter=6"), (dict(filter=-1), "filter=-1"),
    (dict(ld=59), "row stride 59"), (dict(B=2, bs=100), "image stride 100"), (dict(work=257), "256-byte aligned"), (dict(work=None), "work"),
    (dict(work_bytes=1000), "work holds 1000"), (dict(out_cap=62), "out_cap=62"), (dict(px=None), "px must not be NULL"),
    (dict(n_dev=12), "8-byte aligned"),
])
def test_c_entry_refuses_by_name_before_any_launch(kw, match):
    import re

    from fluxmi import _lib

    a = dict(px=4096, ld=60, bs=540, B=1, H=9, W=20, C=3, filter=5, work=4096, work_bytes=1 << 40, out=4096, out_cap=1 << 20, n_dev=4096)
    a.update(kw)
    rc = _lib.lib.fluxmi_png_encode(a["px"], a["ld"], a["bs"], a["B"], a["H"], a["W"], a["C"], a["filter"], a["work"], a["work_bytes"],
                                    a["out"], a["out_cap"], a["n_dev"], None)
    assert rc != 0 and re.search(match, _lib.lib.fluxmi_last_error().decode()), _lib.lib.fluxmi_last_error()


def test_python_refusals_and_the_pipelines_choice():
    import util
    from flux_pipeline import PNG_ENCODERS, FluxPipeline
    from fluxmi import ops

    for kw, match in ((dict(filter="best"), "filter='best'"), (dict(C_=2), "2 channels"), (dict(B=2 ** 20, H=2 ** 12), "2\\^31")):
        with pytest.raises(ValueError, match=match):
            ops.png_params(**dict(dict(B=1, H=8, W=8), **kw))
    assert PNG_ENCODERS == ("native", "pil") and util.ModelSpec.model_fields["png_encoder"].default == "native"
    p = object.__new__(FluxPipeline)
    p.upscaler, p.ae = None, object()
    for kw in (dict(output_type="png"), dict(output_type="jpeg"), dict(output_type="latent")):
        with pytest.raises(ValueError, match="png_encoder='webp'"):
            p.generate("a prompt", png_encoder="webp", **kw)
    with pytest.raises(ValueError, match="IDAT"):
        p.generate("a prompt", output_type="png", num_images=64, height=16384, width=16384)
    p.config = type("Cfg", (), {"png_encoder": "pil"})()
    assert p._png_encoder(None) == "pil" and p._png_encoder("native") == "native"


def test_http_answers_image_png():
    from fastapi.testclient import TestClient

    import api

    calls = []

    class Stub:
        def generate(self, **kw):
            calls.append(kw)
            return io.BytesIO(b"\x89PNG" if kw.get("output_type") == "png" else b"\xff\xd8")

    api.app.state.model = Stub()
    c = TestClient(api.app)
    r = c.post("/generate", json={"prompt": "x"})
    assert r.headers["content-type"] == "image/jpeg" and "output_type" not in calls[-1] and "png_encoder" not in calls[-1]
    r = c.post("/generate", json={"prompt": "x", "output_type": "png", "png_encoder": "pil"})
    assert r.status_code == 200 and r.headers["content-type"] == "image/png" and r.content == b"\x89PNG"
    assert calls[-1]["output_type"] == "png" and calls[-1]["png_encoder"] == "pil"
    assert c.post("/generate", json={"prompt": "x", "output_type": "webp"}).status_code == 422
    lines = c.post("/generate", json={"prompt": "x", "output_type": "png", "stream": True}).text.splitlines()
    import base64
    import json

    assert base64.b64decode(json.loads(lines[-1])["image"]) == b"\x89PNG"
