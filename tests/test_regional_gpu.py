"""Regional prompts (token-group attention masks through the engine) on the GPU: 64^2 .. 128^2 images, the hidden-256 synthetic model.
Every attention of a regional forward is F.scaled_dot_product_attention(q, k, v, attn_mask=allowed) with `allowed` from the descriptor table
(flux_pipeline.build_region_groups); the oracle runs FluxOracle's unchanged blocks with that masked SDPA in place of `attention`.
Helpers are those of tests/test_cfg_gpu.py, imported."""
import io

import pytest
import torch
import torch.nn.functional as F

import attention_mask_ref as mr
import flux_oracle as fo
from test_cfg_gpu import (KNOB_SETS, QUANTS, SCALE, build, cond_kw, dup, inputs, make_oracle, prompts, rel_l2, tiny_config, tiny_pipeline, to_dev)

pytestmark = pytest.mark.gpu

RT = 16  # regional tokens per region in these tests


def region_inputs(kind, params, H, W, Lt, B, seed):
    """test_cfg_gpu.inputs with two regions' text rows appended to both text streams (Lt base rows + 2 x RT) and the tables of both branches"""
    from flux_pipeline import build_region_groups

    d = inputs(kind, params, H, W, Lt, B, seed)
    g = torch.Generator().manual_seed(900 + seed)
    rows = (0.1 * torch.randn(1, 2 * RT, d["txt"].shape[2], generator=g)).to(d["txt"].dtype).expand(B, -1, -1)
    d["txt"], d["neg_txt"] = torch.cat((d["txt"], rows), 1), torch.cat((d["neg_txt"], rows), 1)
    d["txt_ids"] = torch.zeros(B, Lt + 2 * RT, 3, dtype=d["txt_ids"].dtype)
    h, w = H // 16, W // 16
    ys, xs = torch.arange(h)[:, None], torch.arange(w)[None, :]
    grids = torch.stack(((xs < (2 * w + 2) // 3).expand(h, w), ((xs >= w // 3) & (ys >= h // 4)).expand(h, w)))
    n_ref = d["seq"].shape[1] if "seq" in d else 0
    d["groups"] = build_region_groups(Lt, RT, grids, n_ref=n_ref)[None]
    d["groups2"] = torch.stack((d["groups"][0], build_region_groups(Lt, RT, grids, n_ref=n_ref, negative=True)))
    return d


def denoise(model, d, ts, guided=False, use_graph=True, img=None, regional=True):
    kw = dict(cond_kw(d))
    if guided:
        kw.update(neg_txt=d["neg_txt"], neg_y=d["neg_y"], cfg_scale=SCALE)
    if regional:
        kw["attn_groups"] = d["groups2"] if guided else d["groups"]
    return model.denoise(d["img"] if img is None else img, d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts, guidance=3.5, use_graph=use_graph, **kw)


def python_loop(model, d, ts, x, mode, guided):
    """Flux.forward(attn_groups=) per step and the torch expression of the update"""
    B = x.shape[0]
    n = 2 * B if guided else B
    two = dup if guided else (lambda t: t)
    g = torch.full((n,), 3.5, dtype=torch.bfloat16, device=x.device)
    kw = {k: two(v) for k, v in cond_kw(d).items()}
    txt = torch.cat((d["txt"], d["neg_txt"]), 0) if guided else d["txt"]
    y = torch.cat((d["y"], d["neg_y"]), 0) if guided else d["y"]
    groups = d["groups2"].repeat_interleave(B, 0) if guided else d["groups"]
    for t_curr, t_prev in zip(ts[:-1], ts[1:]):
        tv = torch.full((n,), t_curr, dtype=torch.bfloat16, device=x.device)
        pred = model(two(x), two(d["img_ids"]), txt, two(d["txt_ids"]), tv, y, g, mode=mode, attn_groups=groups, **kw)
        x = x + (t_prev - t_curr) * ((pred[B:] + SCALE * (pred[:B] - pred[B:])) if guided else pred)
    return x


STREAMS = [("plain", False), ("plain", True), ("fill", False), ("kontext", False)]


@pytest.mark.parametrize("kind,guided", STREAMS, ids=["plain", "guided", "fill", "kontext"])
@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_regional_denoise_bit_exact(dev, qname, kind, guided):
    """engine graph loop == eager loop == a Python loop over Flux.forward(attn_groups=), bit for bit; fp8 also under the tuning knob sets"""
    from fluxmi import _lib

    cfg = tiny_config(kind)
    model, _ = build(cfg, QUANTS[qname], dev)
    B, H, W, Lt = 2, 64, 96, 32
    d = to_dev(region_inputs(kind, cfg.params, H, W, Lt, B, seed=5), dev)
    ts = fo.get_schedule(16, d["img"].shape[1])
    lat = denoise(model, d, ts[:14], guided, use_graph=False)  # fp8: 13 calibrating regional steps, then frozen
    assert lat.shape == d["img"].shape and torch.isfinite(lat).all()
    ts2 = ts[:7]
    a = denoise(model, d, ts2, guided, img=lat)
    b = denoise(model, d, ts2, guided, img=lat, use_graph=False)
    assert torch.equal(a, b), f"graph vs eager: rel-L2 {rel_l2(a, b):.3e}"
    c = python_loop(model, d, ts2, lat.clone(), 1 if qname == "fp8" else 2, guided)
    assert torch.equal(a, c), f"graph loop vs python loop: rel-L2 {rel_l2(a, c):.3e}"
    assert not torch.equal(a, denoise(model, d, ts2, guided, img=lat, regional=False)), "the table has no effect"
    if qname == "fp8":
        for knobs in KNOB_SETS:
            with _lib.tuning(**knobs):
                a3 = denoise(model, d, ts2, guided, img=lat)
            assert torch.equal(a, a3), f"regional latents change under tuning {knobs}: rel-L2 {rel_l2(a3, a):.3e}"


@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_regional_plain_regional_on_one_engine(dev, qname):
    """regional, plain, regional (another table), guided regional requests of one prepared shape on ONE engine == fresh engines, bit for bit;
    the dense request is the same before and after a regional one; the table's contents are device data of one graph"""
    cfg = tiny_config()
    model, _ = build(cfg, QUANTS[qname], dev)
    d2 = to_dev(region_inputs("plain", cfg.params, 64, 64, 32, 2, seed=5), dev)
    d1 = {k: (v[:1] if k not in ("groups", "groups2") else v) for k, v in d2.items()}
    ts = fo.get_schedule(16, d2["img"].shape[1])
    lat = denoise(model, d2, ts[:14], use_graph=False, regional=False)
    ts2 = ts[:7]
    other = dict(d2, groups=mr.to_i32(mr.table_stripes(d2["groups"].shape[1]))[None].to(dev))
    dense_before = denoise(model, d2, ts2, img=lat, regional=False)
    runs = [lambda: denoise(model, d2, ts2, img=lat), lambda: denoise(model, d2, ts2, img=lat, regional=False),
            lambda: denoise(model, other, ts2, img=lat), lambda: denoise(model, d1, ts2, guided=True, img=lat[:1]),
            lambda: denoise(model, d2, ts2, img=lat)]
    got = [r() for r in runs]
    assert torch.equal(got[1], dense_before), "a request without a table changed after a regional request"
    assert torch.equal(got[0], got[4]) and not torch.equal(got[0], got[2]) and not torch.equal(got[0], got[1])
    for i, r in enumerate(runs):
        model._invalidate_engine()
        fresh = r()
        assert torch.equal(got[i], fresh), f"request {i} on the shared engine differs from a fresh engine: rel-L2 {rel_l2(got[i], fresh):.3e}"


def test_engine_refuses_a_row_without_self_admission_and_counts_the_table(dev):
    """a bad table is refused; a good one goes into the engine's own workspace buffer "attn_groups": [B, L] x 4 bytes of the workspace
    allocation, which fluxmi_engine_workspace_bytes sums with the engine's other allocations"""
    import ctypes as C

    from fluxmi import _lib

    cfg = tiny_config()
    model, _ = build(cfg, None, dev)
    d = to_dev(region_inputs("plain", cfg.params, 64, 64, 32, 1, seed=3), dev)
    ts = fo.get_schedule(4, d["img"].shape[1])
    bad = d["groups"].clone()
    bad[0, 3] = int(mr.to_i32(mr.desc(torch.tensor(0), torch.tensor(0b10))))
    with pytest.raises(RuntimeError, match="does not admit its own key group"):
        denoise(model, dict(d, groups=bad), ts)
    with pytest.raises(ValueError, match="attn_groups"):
        denoise(model, dict(d, groups=d["groups"][:, :-1]), ts)
    out = denoise(model, d, ts)
    assert torch.isfinite(out).all()
    n, nb, ptr, p0, n0 = C.c_longlong(), C.c_longlong(), C.c_void_p(), C.c_void_p(), C.c_longlong()
    _lib.call("fluxmi_engine_workspace_bytes", model._engine, C.byref(n))
    _lib.call("fluxmi_engine_get_buffer", model._engine, b"attn_groups", C.byref(ptr), C.byref(nb))
    _lib.call("fluxmi_engine_get_buffer", model._engine, b"ids", C.byref(p0), C.byref(n0))
    B, L = d["groups"].shape
    assert nb.value == B * L * 4, f"the engine's table buffer holds {nb.value} bytes, [B, L] descriptors are {B * L * 4}"
    # the table lies in the workspace allocation, behind the buffer "ids" of the same allocation and within the bytes reported
    assert 0 < ptr.value - p0.value and ptr.value - p0.value + nb.value <= n.value
    assert ptr.value != d["groups"].data_ptr()


def masked_attention(allowed):
    """fo.attention with attn_mask=allowed [B, L, L] (exact=True: fo.attention_exact's fp64 softmax over the allowed keys)"""
    def sdpa(q, k, v, pe):
        q, k = fo.apply_rope(q, k, pe)
        x = F.scaled_dot_product_attention(q, k, v, attn_mask=allowed[:, None]).transpose(1, 2)
        return x.reshape(*x.shape[:-2], -1)

    def exact(q, k, v, pe):
        q, k = fo.apply_rope(q, k, pe)
        s = (q.double() @ k.double().transpose(-1, -2)) / (q.shape[-1] ** 0.5)
        x = (torch.softmax(s.masked_fill(~allowed[:, None], -float("inf")), dim=-1) @ v.double()).to(q.dtype).transpose(1, 2)
        return x.reshape(*x.shape[:-2], -1)

    return sdpa, exact


def test_regional_denoise_matches_oracle(dev, monkeypatch):
    """B = 1, 64 x 64, 16 steps through calibration.  The oracle: FluxOracle's blocks with a masked SDPA.  Gates as in tests/test_cfg_gpu.py:
    fp8 flows: rel-L2(engine, oracle-bf16) <= 1.25 x rel-L2(oracle-fp8, oracle-bf16); bf16 flow: <= max(1e-2, 1.75 x floor), floor = the
    oracle's own movement when its masked SDPA is evaluated in fp64 (attention vs attention_exact, recomputed with the mask)."""
    H, W, Lt, B, n = 64, 64, 32, 1, 16
    ts = fo.get_schedule(n, (H // 16) * (W // 16))
    ref = {}
    for qname in QUANTS:
        cfg = tiny_config()
        model, sd = build(cfg, QUANTS[qname], dev)
        inp = region_inputs("plain", cfg.params, H, W, Lt, B, seed=7)
        sdpa, exact = masked_attention(mr.allowed_of(inp["groups"]))
        run = lambda q, fn: _oracle_loop(make_oracle(cfg, sd, q), inp, ts, fn, monkeypatch)
        if not ref:
            ref["o16"] = run(None, sdpa)
            ref["floor16"] = rel_l2(run(None, exact), ref["o16"])
            dense = fo.denoise(make_oracle(cfg, sd, None), inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], ts, guidance=3.5)
            assert rel_l2(dense, ref["o16"]) > 2 * max(1e-2, 1.75 * ref["floor16"]), "the mask must matter: the dense oracle has to miss the gate by far"
        got = denoise(model, to_dev(inp, dev), ts)
        assert torch.isfinite(got).all()
        e16 = rel_l2(got, ref["o16"])
        if qname == "bf16":
            gate = max(1e-2, 1.75 * ref["floor16"])
            print(f"[regional bf16] engine vs oracle-bf16 {e16:.3e}; floor (masked attention vs masked attention_exact) {ref['floor16']:.3e}; gate {gate:.3e}")
            assert e16 <= gate, f"bf16: rel-L2 {e16:.3e} > max(1e-2, 1.75 x {ref['floor16']:.3e})"
        else:
            yard = rel_l2(run(QUANTS[qname], sdpa), ref["o16"])
            print(f"[regional {qname}] engine vs oracle-bf16 {e16:.3e}; yardstick (oracle-fp8 vs oracle-bf16) {yard:.3e}; ratio {e16 / yard:.3f} (gate 1.25)")
            assert e16 <= 1.25 * yard, f"{qname}: vs bf16 flow {e16:.3e} > 1.25 x {yard:.3e}"


def _oracle_loop(oracle, inp, ts, attn_fn, monkeypatch):
    with monkeypatch.context() as mp:
        mp.setattr(fo, "attention", attn_fn)
        return fo.denoise(oracle, inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], ts, guidance=3.5)


# ---- pipeline --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe(dev):
    p = tiny_pipeline(dev)
    p.compile()
    assert p.model.calibration_state()[0]
    return p


def region_prompts():
    g = torch.Generator().manual_seed(2)
    return [{"txt": 0.1 * torch.randn(1, 32, 128, generator=g), "vec": torch.randn(1, 64, generator=g)} for _ in range(2)]


def test_pipeline_regions(dev, pipe):
    from flux_pipeline import build_region_groups, region_token_grid

    pos, neg = prompts()
    ra, rb = region_prompts()
    kw = dict(width=128, height=64, num_steps=6, seed=7, silent=True, output_type="latent", regional_tokens=RT)
    box_a, box_b, box_a2 = (0.0, 0.0, 0.5, 1.0), (0.5, 0.0, 1.0, 1.0), (0.25, 0.0, 0.75, 1.0)
    plain = pipe.generate(pos, **kw)
    reg = pipe.generate(pos, regions=[{"prompt": ra, "box": box_a}, {"prompt": rb, "box": box_b}], **kw)
    assert reg.shape == plain.shape and torch.isfinite(reg).all() and not torch.equal(reg, plain)
    assert torch.equal(pipe.generate(pos, **kw), plain), "a request without regions changed after a regional one"
    # == model.denoise on prepare's tensors + the table
    generator, _ = pipe.set_seed(7)
    noise, ts = pipe.preprocess_latent(height=64, width=128, num_steps=6, generator=generator, num_images=1)
    img, img_ids, vec, txt, txt_ids = map(lambda x: x.contiguous(), pipe.prepare(noise, pos))
    rows = torch.cat([pipe.prepare(noise, r)[3][:, :RT] for r in (ra, rb)], 1)
    grids = torch.stack([region_token_grid({"prompt": "", "box": b}, 64, 128) for b in (box_a, box_b)])
    tab = build_region_groups(txt.shape[1], RT, grids)[None].to(dev)
    txt2 = torch.cat((txt, rows), 1).contiguous()
    want = pipe.model.denoise(img, img_ids, txt2, torch.zeros(1, txt2.shape[1], 3, device=dev, dtype=txt_ids.dtype), vec, ts, guidance=3.5, attn_groups=tab)
    assert torch.equal(reg, pipe.unpack(want.float(), 64, 128))
    # moving region A's box changes the output ...
    moved = pipe.generate(pos, regions=[{"prompt": ra, "box": box_a2}, {"prompt": rb, "box": box_b}], **kw)
    d_moved = rel_l2(moved, reg)
    # ... listing the two regions in the other order does not, beyond rounding: it permutes text rows of the joint sequence (every other
    # operator is per row), so only attention's summation order changes -- held to the 1e-2 floor the bf16 rounding-level gates of
    # tests/test_cfg_gpu.py use, and far below what moving a box does
    swapped = pipe.generate(pos, regions=[{"prompt": rb, "box": box_b}, {"prompt": ra, "box": box_a}], **kw)
    d_swap = rel_l2(swapped, reg)
    print(f"[regions] moved box: rel-L2 {d_moved:.3e}; regions listed in the other order: {d_swap:.3e}")
    assert d_swap <= 1e-2 and d_moved > 10 * d_swap and d_moved > 1e-2
    # a mask image instead of a box; with a negative prompt; refusals
    m = torch.zeros(64, 128, dtype=torch.uint8)
    m[:, :64] = 255
    assert torch.equal(pipe.generate(pos, regions=[{"prompt": ra, "mask": m}, {"prompt": rb, "box": box_b}], **kw), reg)
    gd = pipe.generate(pos, regions=[{"prompt": ra, "box": box_a}, {"prompt": rb, "box": box_b}], negative_prompt=neg, true_cfg_scale=SCALE, **kw)
    assert torch.isfinite(gd).all() and not torch.equal(gd, reg)
    with pytest.raises(ValueError, match="covers no image token"):
        pipe.generate(pos, regions=[{"prompt": ra, "box": (0.0, 0.0, 0.01, 0.01)}], **kw)
    with pytest.raises(ValueError, match="multiple of 16"):
        pipe.generate(pos, regions=[{"prompt": ra, "box": box_a}], **{**kw, "regional_tokens": 24})
    with pytest.raises(ValueError, match="exactly one of"):
        pipe.generate(pos, regions=[{"prompt": ra}], **kw)


def test_http_regions_contract():
    """/generate accepts `regions` (+ `regional_tokens`), passes them on only when set, and rejects malformed ones with 4xx"""
    from fastapi.testclient import TestClient

    import api

    calls = []

    class Stub:
        def generate(self, **kw):
            calls.append(kw)
            return io.BytesIO(b"\xff\xd8jpeg-bytes\xff\xd9")

    api.app.state.model = Stub()
    c = TestClient(api.app)
    base = {"prompt": "a meadow", "width": 512, "height": 512, "num_steps": 4, "seed": 7}
    assert c.post("/generate", json=base).status_code == 200
    assert "regions" not in calls[-1] and "regional_tokens" not in calls[-1]
    regs = [{"prompt": "a red fox", "box": [0.0, 0.0, 0.5, 1.0]}, {"prompt": "a snowy owl", "mask": "owl_mask.png"}]
    r = c.post("/generate", json={**base, "regions": regs, "regional_tokens": 64})
    assert r.status_code == 200 and r.content.startswith(b"\xff\xd8")
    assert calls[-1]["regional_tokens"] == 64 and len(calls[-1]["regions"]) == 2
    assert calls[-1]["regions"][0] == {"prompt": "a red fox", "box": (0.0, 0.0, 0.5, 1.0)} and calls[-1]["regions"][1] == {"prompt": "a snowy owl", "mask": "owl_mask.png"}
    n = len(calls)
    for bad in ([], [{"box": [0, 0, 1, 1]}], [{"prompt": "x"}], [{"prompt": "x", "box": [0, 0, 1, 1], "mask": "m.png"}], [{"prompt": "x", "box": [0, 0, 1]}],
                [{"prompt": "x", "box": [0.5, 0, 0.2, 1]}], [{"prompt": "x", "box": [0, 0, 1.5, 1]}], "left", [{"prompt": 3, "box": [0, 0, 1, 1]}]):
        assert 400 <= c.post("/generate", json={**base, "regions": bad}).status_code < 500, f"regions={bad!r} accepted"
    assert 400 <= c.post("/generate", json={**base, "regions": regs, "regional_tokens": 24}).status_code < 500
    assert len(calls) == n, "a malformed request reached generate()"
