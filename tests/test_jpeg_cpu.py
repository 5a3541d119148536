"""The JPEG definition without a GPU: tests/jpeg_ref.py (the definition of include/fluxmi.h in numpy) against Pillow on libjpeg-turbo, the
coverage of the device test's case list, the teeth of that comparison, and the host-side pieces of the native encoder (header, refusals)."""
import io
import os
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "flux-fp8-api_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import jpeg_cases as jc  # noqa: E402
import jpeg_ref as jr  # noqa: E402

PIL_SIZES = [(16, 16), (17, 33), (250, 130)]  # W x H
PIL_QUALITIES = [1, 50, 75, 90, 99, 100]


def _pillow(im: np.ndarray, **kw) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(im).save(buf, format="JPEG", **kw)
    return buf.getvalue()


# ---- 1. decodability --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", ["4:2:0", "4:4:4"])
@pytest.mark.parametrize("R", [0, 1, 5])
def test_pillow_opens_every_reference_stream(ss, R):
    for (W, H) in jc.SIZES:
        for B in (1, 3):
            im = jc.make_image("photo", B, H, W, seed=W + H)
            got = Image.open(io.BytesIO(jr.jpeg_ref(im, 90, ss, R)))
            got.load()
            assert got.size == (W, B * H) and got.mode == "RGB"
            want = [(2, 2), (1, 1), (1, 1)] if ss == "4:2:0" else [(1, 1)] * 3
            assert [layer[1:3] for layer in got.layer] == want


# ---- 2. against Pillow --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", ["4:2:0", "4:4:4"])
@pytest.mark.parametrize("q", PIL_QUALITIES)
@pytest.mark.parametrize("size", PIL_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_equals_pillow_byte_for_byte(size, q, ss):
    """Byte equality holds on Pillow 12.2 / libjpeg-turbo: the entropy-coded segment (end of SOS .. EOI), both DQT payloads and the four DHT
    payloads.  It holds at every size only with libjpeg's two edge rules in the definition (the last CHROMA row repeats below a 4:2:0 image;
    Y blocks of an MCU that hold no image pixel are dummy blocks): see include/fluxmi.h, "Edges"."""
    W, H = size
    for fam in ("photo", "noise"):
        im = jc.make_image(fam, 1, H, W, seed=q)[0]
        pil, ref = _pillow(im, quality=q, subsampling=ss), jr.jpeg_ref(im, q, ss, 0)
        assert jr.segments(pil, 0xDB) == jr.segments(ref, 0xDB), "quantisation tables"
        assert sorted(jr.segments(pil, 0xC4)) == sorted(jr.segments(ref, 0xC4)), "Huffman tables"
        assert jr.scan_bytes(pil) == jr.scan_bytes(ref), f"{fam}: the entropy-coded segments differ"


@pytest.mark.parametrize("ss", ["4:2:0", "4:4:4"])
@pytest.mark.parametrize("R", [1, 3, 40])
def test_reference_restarts_equal_pillow(ss, R):
    """Pillow's restart_marker_blocks counts MCUs, like restart_interval: the same DRI payload and the same scan, RST markers included"""
    for (W, H) in PIL_SIZES:
        im = jc.make_image("noise", 1, H, W, seed=R)[0]
        pil, ref = _pillow(im, quality=90, subsampling=ss, restart_marker_blocks=R), jr.jpeg_ref(im, 90, ss, R)
        assert jr.segments(pil, 0xDD) == jr.segments(ref, 0xDD) == [R.to_bytes(2, "big")]
        assert jr.scan_bytes(pil) == jr.scan_bytes(ref)


def test_default_request_is_what_pillow_writes_today():
    """quality 99 and nothing else, as FluxPipeline._jpeg saves: 4:2:0, and the reference's scan"""
    im = jc.make_image("photo", 1, 48, 64, seed=5)[0]
    pil = _pillow(im, quality=99)
    assert [layer[1:3] for layer in Image.open(io.BytesIO(pil)).layer] == [(2, 2), (1, 1), (1, 1)]
    assert jr.scan_bytes(pil) == jr.scan_bytes(jr.jpeg_ref(im, 99, "4:2:0", 0))


# ---- 3. the case list of the device test covers every path ----------------------------------------------------------------------------------
def test_case_list_covers_every_path():
    stats = [jc.reference_of(c)[1] for c in jc.CASES]
    assert any(s["zrl"] > 0 for s in stats), "no ZRL"
    assert any(s["blocks_without_eob"] > 0 for s in stats), "no block whose level 63 is non-zero"
    assert any(s["stuffed_ff"] > 0 for s in stats), "no stuffed 0xFF"
    seen = set()
    for s in stats:
        seen |= set(s["rst"])
    assert seen == set(range(8)), f"RSTm seen: {sorted(seen)}"
    assert any(len(s["rst"]) > 8 for s in stats), "no restart count wraps past 7"
    assert max(s["max_dc_category"] for s in stats) == 11, "no DC difference of category 11"
    assert max(s["max_ac_category"] for s in stats) == 10, "no AC level of category 10"
    assert any(s["eob_only_blocks"] > 0 for s in stats), "no EOB-only block"
    assert any(s["replicated_right"] for s in stats) and any(s["replicated_bottom"] for s in stats)
    # the axes of the issue's product all occur
    assert {(c[3], c[2]) for c in jc.CASES} >= set(jc.SIZES)
    assert {c[4] for c in jc.CASES} >= {1, 50, 90, 99, 100} and {c[5] for c in jc.CASES} == {"4:2:0", "4:4:4"}
    assert {c[1] for c in jc.CASES} == {1, 3} and {c[0] for c in jc.CASES} >= {"noise", "ramp", "impulse", "const0", "const255", "checker8"}
    rs = {c[6] for c in jc.CASES}
    assert rs >= {0, 1, 3, None} and any(r is not None and r > -(-c[3] // 8) * -(-c[1] * c[2] // 8) for c in jc.CASES for r in [c[6]])
    assert any(c[1] == 3 and c[2] % 16 for c in jc.CASES), "no stacked batch that crosses an MCU row"
    for c in jc.BIG_CASES:
        assert jc.reference_of(c)[0].count(b"\xFF\xD0") > 10


# ---- 4. teeth -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutation", ["mutate_bias_2", "mutate_swap_cbcr", "mutate_rst_no_wrap"])
def test_a_wrong_encoder_changes_the_bytes(mutation):
    changed = [c for c in jc.CASES if jr.jpeg_ref(jc.image_of(c), c[4], c[5], jc.restart_of(c), **{mutation: True}) != jc.reference_of(c)[0]]
    assert changed, f"{mutation} changes no case of the list"


# ---- 5. the native encoder's host side --------------------------------------------------------------------------------------------------------
def test_c_abi_and_header_bytes():
    from fluxmi import _lib, ops

    hdr = open(os.path.join(ROOT, "include", "fluxmi.h")).read()
    for name in ("fluxmi_jpeg_workspace_bytes", "fluxmi_jpeg_encode", "fluxmi_jpeg_finish", "fluxmi_jpeg_header"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name) and f"int {name}(" in hdr
    assert _lib.lib.fluxmi_abi_version() == 5 and _lib.ABI_VERSION == 5
    assert len(_lib.lib.fluxmi_jpeg_encode.argtypes) == 14 and len(_lib.lib.fluxmi_jpeg_workspace_bytes.argtypes) == 7
    assert ops.JPEG_DEFAULT_RESTART == jc.DEFAULT_RESTART
    for k, v in (("FLUXMI_JPEG_RESTART_420", 4), ("FLUXMI_JPEG_RESTART_444", 8), ("FLUXMI_JPEG_420", 0), ("FLUXMI_JPEG_444", 1)):
        assert f"#define {k} {v}\n" in hdr
    # the header the host writes (the C++ copies of the Annex K tables, the quality rule) is the reference's, byte for byte
    for (B, H, W, q, ss, R) in [(1, 16, 16, 99, "4:2:0", None), (3, 33, 17, 1, "4:4:4", 0), (1, 130, 250, 50, "4:2:0", 3), (2, 5, 7, 100, "4:4:4", 60000),
                                (1, 65535, 65535, 75, "4:2:0", 65535)] + [(1, 8, 8, q, "4:2:0", 0) for q in range(1, 101)]:
        want = jr.header(B * H, W, q, ss, ops.JPEG_DEFAULT_RESTART[ss] if R is None else R)
        assert ops.jpeg_header(B, H, W, q, ss, R) == want
    # the slot of an interval is sized by the worst case of a block
    work, cap = ops.jpeg_workspace_bytes(1, 16, 16, "4:2:0", 0)
    assert cap >= len(jr.header(16, 16, 99, "4:2:0", 0)) + 6 * 416 + 2 and work >= 6 * 64 * 2 + 6 * 416


@pytest.mark.parametrize("kw, match", [
    (dict(W=65536), "65535"),
    (dict(B=2, H=32768), "65535"),
    (dict(quality=0), "quality=0"),
    (dict(quality=101), "quality=101"),
    (dict(quality=True), "quality=True"),
    (dict(subsampling="4:2:2"), "4:2:2"),
    (dict(restart_interval=-1), "restart_interval=-1"),
    (dict(restart_interval=65536), "restart_interval=65536"),
])
def test_refusals_by_name(kw, match):
    from fluxmi import ops

    a = dict(B=1, H=16, W=16, quality=99, subsampling="4:2:0", restart_interval=None)
    a.update(kw)
    with pytest.raises(ValueError, match=match):
        ops.jpeg_params(**a)


def test_c_entries_refuse_by_name():
    import ctypes as C

    from fluxmi import _lib

    work, cap = C.c_longlong(0), C.c_longlong(0)
    assert _lib.lib.fluxmi_jpeg_workspace_bytes(1, 70000, 8, 0, 0, C.byref(work), C.byref(cap)) != 0
    assert b"65535" in _lib.lib.fluxmi_last_error()
    assert _lib.lib.fluxmi_jpeg_workspace_bytes(1, 8, 8, 2, 0, C.byref(work), C.byref(cap)) != 0
    assert b"subsampling=2" in _lib.lib.fluxmi_last_error()
    # NULL operands and an out that cannot hold the header are refused before any launch
    assert _lib.lib.fluxmi_jpeg_encode(None, 24, 192, 1, 8, 8, 99, 0, 0, None, None, 0, None, None) != 0
    assert b"rgb must not be NULL" in _lib.lib.fluxmi_last_error()


# ---- 6. the pipeline's and the HTTP layer's choice of encoder ------------------------------------------------------------------------------
def test_pipeline_refusals_fire_up_front():
    import util
    from flux_pipeline import JPEG_ENCODERS, FluxPipeline

    assert JPEG_ENCODERS == ("pil", "native") and util.ModelSpec.model_fields["jpeg_encoder"].default == "pil"
    p = object.__new__(FluxPipeline)
    p.upscaler, p.ae = None, object()
    with pytest.raises(ValueError, match="jpeg_encoder='webp'"):
        p.generate("a prompt", jpeg_encoder="webp")
    with pytest.raises(ValueError, match="jpeg_encoder='webp'"):
        p.generate("a prompt", jpeg_encoder="webp", output_type="latent")
    with pytest.raises(ValueError, match="65535"):
        p.generate("a prompt", jpeg_encoder="native", num_images=4100, height=16, width=16)
    with pytest.raises(ValueError, match="65535"):
        p.generate("a prompt", jpeg_encoder="native", height=16, width=65536 + 16)
    with pytest.raises(ValueError, match="quality=0"):
        p.generate("a prompt", jpeg_encoder="native", jpeg_quality=0)
    # the configuration's value is the default of a request that does not say
    p.config = type("Cfg", (), {"jpeg_encoder": "native"})()
    assert p._jpeg_encoder(None) == "native" and p._jpeg_encoder("pil") == "pil"
    p.config.jpeg_encoder = "turbo"
    with pytest.raises(ValueError, match="jpeg_encoder='turbo'"):
        p.generate("a prompt")


def test_http_jpeg_encoder_field():
    from fastapi.testclient import TestClient

    import api

    assert api.GenerateArgs.model_fields["jpeg_encoder"].default is None
    assert "jpeg_encoder" in api.GenerateArgs.model_json_schema()["properties"]
    calls = []

    class Stub:
        def generate(self, **kw):
            calls.append(kw)
            return io.BytesIO(b"\xff\xd8jpeg\xff\xd9")

    api.app.state.model = Stub()
    c = TestClient(api.app)
    assert c.post("/generate", json={"prompt": "x"}).status_code == 200
    assert "jpeg_encoder" not in calls[-1]  # a request that does not ask is the request it was
    assert c.post("/generate", json={"prompt": "x", "jpeg_encoder": "native"}).status_code == 200
    assert calls[-1]["jpeg_encoder"] == "native"
    assert c.post("/generate", json={"prompt": "x", "jpeg_encoder": "webp"}).status_code == 422
