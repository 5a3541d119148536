"""Masked-latent inpainting and differential diffusion on the GPU.  Every update of a masked request is ONE kernel (csrc/update_step.hip,
the BLEND arms of euler_kernel): the Euler (or guided Euler) step followed by

    p  = t_next * noise + (1.0 - t_next) * x0
    x' = (1 - m) * p + m * x1                        every operation rounded to bf16 once, python scalars as fp32

(tests/inpaint_util.py).  m == 1 gives x1, m == 0 gives p, and m == 0 at t_next == 0 gives x0: the kept elements of a request whose schedule
ends at 0 are x0 bit for bit.  Model helpers are those of tests/test_cfg_gpu.py."""
import base64
import ctypes as C
import io

import numpy as np
import pytest
import torch

import flux_oracle as fo
import inpaint_util as iu
from test_cfg_gpu import (IN_CHANNELS, KNOB_SETS, LAYOUTS, QUANTS, SCALE, build, cond_kw, dup, inputs, make_oracle, prompts, rel_l2, state_dict,
                          tiny_config, to_dev)

pytestmark = pytest.mark.gpu


# ---- 1. the kernel against the torch expression -------------------------------------------------------------------------------------
TNEXT = [0.7313, 0.40625, 0.0]  # the last step of a request ends at 0
THR = [0.3, 0.75, 0.5]          # 0.3 is no bf16 (nor fp32) number: the compare must be the fp32 one; 0.5 is a mask value (strict compare)


def kernel_masks(B, Rp, Co, g):
    soft = torch.rand(B, Rp, Co, generator=g).to(torch.bfloat16)
    soft[..., 0], soft[..., 1], soft[..., 2], soft[..., 3] = 0.5, 0.30078125, 0.298828125, 0.75  # at and around the thresholds
    return {"soft": soft, "ones": torch.ones_like(soft), "zeros": torch.zeros_like(soft),
            "binary": (torch.rand(B, Rp, Co, generator=g) < 0.5).to(torch.bfloat16)}


@pytest.mark.parametrize("guided", [False, True], ids=["plain_update", "guided_update"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("B", [1, 3])
def test_blend_euler_kernel_bit_exact(dev, layout, B, guided):
    from fluxmi import _lib, ops

    R, Rp, Ci, Co = LAYOUTS[layout]
    g = torch.Generator().manual_seed(31 + B)
    dts = torch.tensor([-0.0625, -0.03173828125, 0.0471], dtype=torch.float32)
    d_dts = dts.to(dev)
    d_tn = torch.tensor(TNEXT, dtype=torch.float32, device=dev)
    d_om = torch.tensor([1.0 - t for t in TNEXT], dtype=torch.float32, device=dev)
    d_thr = torch.tensor(THR, dtype=torch.float32, device=dev)
    d_scale = torch.tensor([SCALE], dtype=torch.float32, device=dev)
    nb = 2 * B if guided else B
    x0, noise = (torch.randn(B, Rp, Co, generator=g).to(torch.bfloat16).to(dev) for _ in range(2))

    def call(img, pred, m, step_ptr, thr_ptr, b=B, rows=R, prows=Rp):
        _lib.call("fluxmi_blend_euler", ops._p(img), ops._p(pred), ops._p(x0), ops._p(noise), ops._p(m), ops._p(d_dts), ops._p(d_tn), ops._p(d_om),
                  thr_ptr, step_ptr, ops._p(d_scale) if guided else None, b, rows, prows, Ci, Co, ops._stream())
        torch.cuda.synchronize()

    for name, m in kernel_masks(B, Rp, Co, g).items():
        m = m.to(dev)
        for step in (0, 2):
            for diff in (False, True):
                # guided: the two halves of the stream start DIFFERENT: the kernel must read x from the prompt half alone and write both
                img = torch.randn(nb, R, Ci, generator=g).to(torch.bfloat16).to(dev)
                pred = torch.randn(nb, Rp, Co, generator=g).to(torch.bfloat16).to(dev)
                before, kept = img.clone(), (x0.clone(), noise.clone(), m.clone(), pred.clone())
                x = img[:B, :Rp, :Co]
                v = (pred[:B], pred[B:]) if guided else pred
                thr = THR[step] if diff else None
                want = iu.blend_step(x, v, float(dts[step]), TNEXT[step], x0, noise, m, thr=thr, scale=SCALE if guided else None)
                assert want.dtype == torch.bfloat16
                x1 = iu.blend_step(x, v, float(dts[step]), TNEXT[step], x0, noise, torch.ones_like(m), scale=SCALE if guided else None)
                d_step = torch.tensor([step], dtype=torch.int32, device=dev)
                call(img, pred, m, ops._p(d_step), ops._p(d_thr) if diff else None)
                tag = f"{layout} B={B} mask={name} step={step} diff={diff}"
                assert torch.equal(img[:B, :Rp, :Co], want), f"{tag}: rel-L2 {rel_l2(img[:B, :Rp, :Co], want):.3e}"
                if guided:
                    assert torch.equal(img[B:, :Rp, :Co], img[:B, :Rp, :Co]), f"{tag}: the halves differ after the update"
                assert torch.equal(img[:, Rp:], before[:, Rp:]), f"{tag}: reference rows changed"
                assert torch.equal(img[..., Co:], before[..., Co:]), f"{tag}: conditioning channels changed"
                assert all(torch.equal(a, b) for a, b in zip(kept, (x0, noise, m, pred))), f"{tag}: an input changed"
                # the exact properties the requests rely on
                m_eff = iu.effective_mask(m, thr)
                assert torch.equal(want[m_eff == 1], x1[m_eff == 1])
                if TNEXT[step] == 0.0:
                    assert torch.equal(want[m_eff == 0], x0[m_eff == 0])
    # step = NULL reads entry 0 of every table
    m = kernel_masks(B, Rp, Co, g)["soft"].to(dev)
    img = torch.randn(nb, R, Ci, generator=g).to(torch.bfloat16).to(dev)
    pred = torch.randn(nb, Rp, Co, generator=g).to(torch.bfloat16).to(dev)
    want = iu.blend_step(img[:B, :Rp, :Co], (pred[:B], pred[B:]) if guided else pred, float(dts[0]), TNEXT[0], x0, noise, m, thr=THR[0],
                         scale=SCALE if guided else None)
    call(img, pred, m, None, ops._p(d_thr))
    assert torch.equal(img[:B, :Rp, :Co], want)
    # malformed shapes are refused with a message, and nothing is written
    before = img.clone()
    with pytest.raises(RuntimeError, match="blend_euler: bad shape"):
        call(img, pred, m, None, None, rows=Rp, prows=R + 1)
    with pytest.raises(RuntimeError, match="blend_euler: bad shape"):
        call(img, pred, m, None, None, b=-1)
    with pytest.raises(RuntimeError, match="blend_euler: NULL argument"):
        _lib.call("fluxmi_blend_euler", ops._p(img), ops._p(pred), None, ops._p(noise), ops._p(m), ops._p(d_dts), ops._p(d_tn), ops._p(d_om),
                  None, None, None, B, R, Rp, Ci, Co, ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(img, before)


def test_blend_euler_kernel_shape_refusals(dev):
    """both shorter and narrower, widths that are no multiple of 8"""
    from fluxmi import _lib, ops

    t = torch.zeros(2, 16, 64, dtype=torch.bfloat16, device=dev)
    f = torch.zeros(4, dtype=torch.float32, device=dev)
    for rows, prows, ci, co in ((16, 8, 64, 32), (16, 16, 64, 12), (16, 16, 60, 60), (16, 16, 32, 64)):
        with pytest.raises(RuntimeError, match="blend_euler: bad shape"):
            _lib.call("fluxmi_blend_euler", ops._p(t), ops._p(t), ops._p(t), ops._p(t), ops._p(t), ops._p(f), ops._p(f), ops._p(f), None, None, None,
                      1, rows, prows, ci, co, ops._stream())


# ---- the request of the model-level tests -----------------------------------------------------------------------------------------------
def denoise(model, d, ts, img=None, inp=None, thr=None, guided=False, **kw):
    if guided:
        kw.update(neg_txt=d["neg_txt"], neg_y=d["neg_y"], cfg_scale=SCALE)
    if inp is not None:
        kw.update(inpaint_x0=inp[0], inpaint_noise=inp[1], inpaint_mask=inp[2], inpaint_thresholds=thr)
    return model.denoise(d["img"] if img is None else img, d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts, guidance=3.5, **cond_kw(d), **kw)


def python_loop(model, d, ts, x, mode, inp, thr=None, guided=False):
    """model(...) per step, the torch expression of the (guided) update, the blend"""
    B = x.shape[0]
    x0, noise, m = inp
    n = 2 * B if guided else B
    two = dup if guided else (lambda t: t)
    g = torch.full((n,), 3.5, dtype=torch.bfloat16, device=x.device)
    kw = {k: two(v) for k, v in cond_kw(d).items()}
    txt, y = (torch.cat((d["txt"], d["neg_txt"]), 0), torch.cat((d["y"], d["neg_y"]), 0)) if guided else (d["txt"], d["y"])
    for i, (t_curr, t_prev) in enumerate(zip(ts[:-1], ts[1:])):
        tv = torch.full((n,), t_curr, dtype=torch.bfloat16, device=x.device)
        pred = model(two(x), two(d["img_ids"]), txt, two(d["txt_ids"]), tv, y, g, mode=mode, **kw)
        v = (pred[:B], pred[B:]) if guided else pred
        x = iu.blend_step(x, v, t_prev - t_curr, t_prev, x0, noise, m, thr=None if thr is None else thr[i], scale=SCALE if guided else None)
    return x


def frozen_request(dev, qname, kind, B=2, seed=5, guided=False):
    """a tiny model calibrated by a 13-step MASKED request at the shape (the calibrating steps run the blend too), then the frozen request
    over the last 8 steps of the schedule, which end at 0: (model, d, ts2, start latents, (x0, noise, mask [1, ...]))"""
    cfg = tiny_config(kind)
    model, sd = build(cfg, QUANTS[qname], dev)
    d = to_dev(inputs(kind, cfg.params, 64, 64, 32, B, seed=seed), dev)
    inp = iu.make_inpaint(B, d["img"].shape[1], 64, seed, device=dev)
    ts = fo.get_schedule(16, d["img"].shape[1])
    lat = denoise(model, d, ts[:14], inp=inp, use_graph=False, guided=guided)
    assert torch.isfinite(lat).all()
    if qname != "bf16":
        assert model.calibration_state()[0]
    assert ts[-1] == 0.0
    return model, d, ts[8:], lat, inp


def ws_bytes(model):
    from fluxmi import _lib

    n = C.c_longlong(0)
    _lib.call("fluxmi_engine_workspace_bytes", model._engine, C.byref(n))
    return n.value


def has_buffer(model, name):
    from fluxmi import _lib

    p = C.c_void_p()
    try:
        _lib.call("fluxmi_engine_get_buffer", model._engine, name.encode(), C.byref(p), None)
    except RuntimeError as e:
        assert "no buffer named" in str(e)
        return False
    return True


# ---- 2. masked denoise: graph == eager == python loop; the exact properties; tuning knobs -------------------------------------------------
@pytest.mark.parametrize("kind", list(IN_CHANNELS))
@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_masked_denoise_bit_exact(dev, qname, kind):
    from fluxmi import _lib

    model, d, ts, lat, inp = frozen_request(dev, qname, kind)
    x0, noise, m = inp
    mode = 1 if qname == "fp8" else 2
    mine = dict(zip(("x0", "noise", "mask"), inp), **{k: d[k] for k in ("seq", "cond") if k in d})
    kept = {k: v.clone() for k, v in mine.items()}
    a = denoise(model, d, ts, img=lat, inp=inp)
    b = denoise(model, d, ts, img=lat, inp=inp, use_graph=False)
    assert a.shape == d["img"].shape and a.dtype == torch.bfloat16
    assert torch.equal(a, b), f"graph vs eager: rel-L2 {rel_l2(a, b):.3e}"
    c = python_loop(model, d, ts, lat.clone(), mode, inp)
    assert torch.equal(a, c), f"graph loop vs python loop: rel-L2 {rel_l2(a, c):.3e}"
    # the schedule ends at 0: every kept element is x0, bit for bit, and the regenerated part moved
    me = m.expand_as(a)
    assert (me == 0).any() and (me == 1).any()
    assert torch.equal(a[me == 0], x0[me == 0]), "a kept element is not the init latent"
    assert not torch.equal(a[me == 1], x0[me == 1]), "no regenerated element differs from the init latent"
    # an all-ones mask is the unmasked request
    plain = denoise(model, d, ts, img=lat)
    ones = denoise(model, d, ts, img=lat, inp=(x0, noise, torch.ones_like(m)))
    assert torch.equal(ones, plain), f"all-ones mask vs no mask: rel-L2 {rel_l2(ones, plain):.3e}"
    assert not torch.equal(a, plain)
    # differential: thresholds that include mask values (0, 1) and split the soft ones
    thr = [1.0 - (i + 1) / (len(ts) - 1) for i in range(len(ts) - 1)]
    assert thr[-1] == 0.0
    da = denoise(model, d, ts, img=lat, inp=inp, thr=thr)
    db = denoise(model, d, ts, img=lat, inp=inp, thr=thr, use_graph=False)
    dc = python_loop(model, d, ts, lat.clone(), mode, inp, thr=thr)
    assert torch.equal(da, db) and torch.equal(da, dc), f"differential: graph vs eager {rel_l2(da, db):.3e}, vs python loop {rel_l2(da, dc):.3e}"
    assert torch.equal(da[me == 0], x0[me == 0]) and not torch.equal(da, a)
    for k, v in kept.items():
        assert torch.equal(mine[k], v), f"the caller's {k} changed"
    if qname == "fp8":
        for knobs in KNOB_SETS:
            with _lib.tuning(**knobs):
                a3 = denoise(model, d, ts, img=lat, inp=inp)
            assert torch.equal(a, a3), f"masked latents change under tuning {knobs}: rel-L2 {rel_l2(a3, a):.3e}"


# ---- 3. the graph is keyed on the blend -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_plain_and_masked_requests_never_share_a_graph(dev, qname):
    cfg = tiny_config()
    model, _ = build(cfg, QUANTS[qname], dev)
    d = to_dev(inputs("plain", cfg.params, 64, 64, 32, 2, seed=5), dev)
    inp = iu.make_inpaint(2, d["img"].shape[1], 64, 5, device=dev)
    ts = fo.get_schedule(16, d["img"].shape[1])
    lat = denoise(model, d, ts[:14], use_graph=False)  # an UNMASKED calibration
    ts2 = ts[8:]
    thr = [0.5] * (len(ts2) - 1)
    first = denoise(model, d, ts2, img=lat)
    assert not has_buffer(model, "inp_x0"), "a request without a mask allocated the inpainting buffers"
    ws = ws_bytes(model)
    runs = [lambda: denoise(model, d, ts2, img=lat), lambda: denoise(model, d, ts2, img=lat, inp=inp),
            lambda: denoise(model, d, ts2, img=lat, inp=inp, thr=thr), lambda: denoise(model, d, ts2, img=lat),
            lambda: denoise(model, d, ts2, img=lat, inp=inp), lambda: denoise(model, d, ts2, img=lat, inp=inp, thr=thr)]
    got = [r() for r in runs]
    assert has_buffer(model, "inp_x0") and ws_bytes(model) == ws + 3 * ((inp[0].numel() * 2 + 255) // 256 * 256)
    assert torch.equal(got[0], first) and torch.equal(got[3], first), "a plain request behind a masked one differs from its earlier result"
    assert torch.equal(got[1], got[4]) and torch.equal(got[2], got[5])
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2])
    for i, r in enumerate(runs[:3]):
        model._invalidate_engine()
        fresh = r()
        assert torch.equal(got[i], fresh), f"request {i} on the shared engine differs from a fresh engine: rel-L2 {rel_l2(got[i], fresh):.3e}"
        assert has_buffer(model, "inp_x0") == (i > 0)


# ---- 4. step caching --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_masked_request_with_step_cache(dev, qname):
    """hits forced by a threshold above every ratio (1e30, the project's value for it: Flux.denoise refuses a non-finite one) and
    cache_max_hits=1: miss, hit, miss, hit, ...  Both tails of the cached step run the blend."""
    model, d, ts, lat, inp = frozen_request(dev, qname, "plain")
    x0, _, m = inp
    ckw = dict(cache_threshold=1e30, cache_max_hits=1)
    a = denoise(model, d, ts, img=lat, inp=inp, **ckw)
    hits = model.step_cache_log()[1]
    assert hits == [i % 2 != 0 for i in range(len(ts) - 1)]
    b = denoise(model, d, ts, img=lat, inp=inp, use_graph=False, **ckw)
    assert model.step_cache_log()[1] == hits
    assert torch.equal(a, b), f"cached masked request, graph vs eager: rel-L2 {rel_l2(a, b):.3e}"
    me = m.expand_as(a)
    assert torch.equal(a[me == 0], x0[me == 0]), "a kept element is not the init latent"
    assert not torch.equal(a, denoise(model, d, ts, img=lat, inp=inp)), "the forced hits changed nothing"


# ---- 5. guidance ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_guided_masked_denoise(dev, qname):
    model, d, ts, lat, inp = frozen_request(dev, qname, "plain", seed=9, guided=True)
    x0, noise, m = inp
    a = denoise(model, d, ts, img=lat, inp=inp, guided=True)
    c = python_loop(model, d, ts, lat.clone(), 1 if qname == "fp8" else 2, inp, guided=True)
    assert torch.equal(a, c), f"guided masked loop vs python loop: rel-L2 {rel_l2(a, c):.3e}"
    assert torch.equal(a, denoise(model, d, ts, img=lat, inp=inp, guided=True, use_graph=False))
    assert not torch.equal(a, denoise(model, d, ts, img=lat, inp=inp)), "the negative branch has no effect"
    me = m.expand_as(a)
    assert torch.equal(a[me == 0], x0[me == 0])
    # a sample's bits do not depend on the batch it rides in
    for b in range(2):
        one = denoise(model, {k: v[b:b + 1] for k, v in d.items()}, ts, img=lat[b:b + 1], inp=(x0[b:b + 1], noise[b:b + 1], m), guided=True)
        assert torch.equal(one[0], a[b]), f"sample {b} depends on its batch: rel-L2 {rel_l2(one[0], a[b]):.3e}"


# ---- 6. against the oracle --------------------------------------------------------------------------------------------------------------
def oracle_masked_loop(oracle, inp, ts, x0, noise, m, guidance=3.5):
    """fo.denoise with the blend behind every update (bf16 tensors, python scalars)"""
    x = inp["img"]
    g = torch.full((x.shape[0],), guidance, dtype=oracle.dtype)
    for t_curr, t_prev in zip(ts[:-1], ts[1:]):
        tv = torch.full((x.shape[0],), t_curr, dtype=oracle.dtype)
        pred = oracle.forward(img=x, img_ids=inp["img_ids"], txt=inp["txt"], txt_ids=inp["txt_ids"], y=inp["y"], timesteps=tv, guidance=g)
        x = iu.blend_step(x, pred, t_prev - t_curr, t_prev, x0, noise, m)
    return x


def test_masked_denoise_matches_oracle(dev, monkeypatch):
    """B = 1, 64 x 64, Lt 32, 16 masked steps through calibration; the oracle loop is fo.denoise's with the blend expression behind every
    update.  The bound is test_cfg_gpu.py::test_guided_denoise_matches_oracle's, unchanged (the blend adds no rounding outside the expression):
    fp8 flows: rel-L2(engine, oracle-bf16 loop) <= 1.25 x rel-L2(oracle-fp8 loop, oracle-bf16 loop);
    bf16 flow: rel-L2(engine, oracle-bf16) <= max(1e-2, 1.75 x floor), floor = the oracle's own movement over the whole loop when its SDPA is
    replaced by fo.attention_exact."""
    H, W, Lt, B, n = 64, 64, 32, 1, 16
    ts = fo.get_schedule(n, (H // 16) * (W // 16))
    ref = {}
    for qname in QUANTS:
        cfg = tiny_config()
        model, sd = build(cfg, QUANTS[qname], dev)
        inp = inputs("plain", cfg.params, H, W, Lt, B, seed=7)
        x0, noise, m = iu.make_inpaint(B, inp["img"].shape[1], 64, 7)
        if not ref:
            ref["o16"] = oracle_masked_loop(make_oracle(cfg, sd, None), inp, ts, x0, noise, m)
            with monkeypatch.context() as mp:
                mp.setattr(fo, "attention", fo.attention_exact)
                ref["o16x"] = oracle_masked_loop(make_oracle(cfg, sd, None), inp, ts, x0, noise, m)
            ref["floor16"] = rel_l2(ref["o16x"], ref["o16"])
        got = denoise(model, to_dev(inp, dev), ts, inp=(x0.to(dev), noise.to(dev), m.to(dev)))
        assert got.shape == inp["img"].shape and torch.isfinite(got).all()
        me = m.expand_as(got).to(dev)
        assert torch.equal(got[me == 0], x0.to(dev)[me == 0])
        e16 = rel_l2(got, ref["o16"])
        if qname == "bf16":
            gate = max(1e-2, 1.75 * ref["floor16"])
            print(f"[inpaint bf16] engine vs oracle-bf16 {e16:.3e}; floor (oracle-bf16, exact attention) {ref['floor16']:.3e}; gate {gate:.3e}")
            assert e16 <= gate, f"bf16: rel-L2 {e16:.3e} > max(1e-2, 1.75 x {ref['floor16']:.3e})"
        else:
            o8 = oracle_masked_loop(make_oracle(cfg, sd, QUANTS[qname]), inp, ts, x0, noise, m)
            yard = rel_l2(o8, ref["o16"])
            print(f"[inpaint {qname}] engine vs oracle-bf16 {e16:.3e}; yardstick (oracle-fp8 vs oracle-bf16) {yard:.3e}; ratio {e16 / yard:.3f} (gate 1.25)")
            assert e16 <= 1.25 * yard, f"{qname}: vs bf16 flow {e16:.3e} > 1.25 x {yard:.3e}"


# ---- 7. pipeline ------------------------------------------------------------------------------------------------------------------------
def tiny_pipeline(dev, in_channels=64):
    """tests/test_cfg_gpu.py's tiny pipeline; in_channels 128 = a Depth / Canny model, 384 = a Fill model"""
    from flux_pipeline import FluxPipeline
    from modules.autoencoder import AutoEncoder, AutoEncoderParams

    cfg = tiny_config()
    if in_channels != 64:
        cfg.params.in_channels, cfg.params.out_channels = in_channels, 64
    cfg.text_enc_max_length = 32
    cfg.ae_device = str(dev)
    cfg.ae_params = AutoEncoderParams(resolution=32, in_channels=3, ch=32, out_ch=3, ch_mult=[1, 2, 2, 2], num_res_blocks=1, z_channels=16,
                                      scale_factor=0.3611, shift_factor=0.1159)
    torch.manual_seed(0)
    ae_sd = {k: v.clone() for k, v in AutoEncoder(cfg.ae_params).state_dict().items()}
    p = FluxPipeline.load_pipeline_from_config(cfg, state_dict=state_dict(cfg.params, 0), ae_state_dict=ae_sd)
    p.compile()
    assert p.model.calibration_state()[0]
    return p


@pytest.fixture(scope="module")
def pipe(dev):
    return tiny_pipeline(dev)


Hpx, Wpx = 96, 64


def photo_and_mask():
    rng = np.random.default_rng(0)
    photo = rng.integers(0, 256, size=(Hpx, Wpx, 3), dtype=np.uint8)
    mask = np.zeros((Hpx, Wpx), dtype=np.uint8)
    mask[24:72, 16:48] = 255
    return photo, mask


def gen(p, prompt, **kw):
    """one request; the VAE encoder's Gaussian sample comes from torch's global generator (img2img's encode), so it is seeded per request"""
    torch.manual_seed(5)
    return p.generate(prompt, width=Wpx, height=Hpx, num_steps=6, seed=7, silent=True, output_type="latent", **kw)


def encoded(p, photo):
    torch.manual_seed(5)
    x = torch.from_numpy(photo).permute(2, 0, 1).contiguous().to(p.device_ae, dtype=p.ae_dtype).div(127.5).sub(1)[None]
    return p.ae.encode(x).to(dtype=p.dtype, device=p.device_flux).float()


def keep_of(mask):
    """latent pixels [H/8, W/8] of a binary pixel mask that are kept (block mean < 0.5)"""
    return torch.from_numpy(mask).float().div(255).reshape(Hpx // 8, 8, Wpx // 8, 8).mean(dim=(1, 3)) < 0.5


def test_pipeline_inpaint(dev, pipe, tmp_path):
    from PIL import Image

    pos, _ = prompts()
    photo, mask = photo_and_mask()
    enc = encoded(pipe, photo)
    keep = keep_of(mask).to(enc.device)
    assert keep.any() and not keep.all()
    a = gen(pipe, pos, init_image=photo, inpaint_mask=mask)
    assert tuple(a.shape) == (1, 16, Hpx // 8, Wpx // 8) and torch.isfinite(a).all()
    assert torch.equal(a[..., keep], enc[..., keep]), "a kept latent pixel is not the encoded init image"
    assert not torch.equal(a[..., ~keep], enc[..., ~keep])
    # every input form of the mask gives the same bytes
    path = str(tmp_path / "mask.png")
    Image.fromarray(mask).save(path)
    buf = io.BytesIO()
    Image.fromarray(mask).save(buf, format="PNG")
    forms = {"PIL": Image.fromarray(mask), "tensor": torch.from_numpy(mask), "RGB array": np.repeat(mask[..., None], 3, -1), "path": path,
             "base64": base64.standard_b64encode(buf.getvalue()).decode(), "data URL": "data:image/png;base64," + base64.standard_b64encode(buf.getvalue()).decode()}
    for name, form in forms.items():
        assert torch.equal(gen(pipe, pos, init_image=photo, inpaint_mask=form), a), f"mask given as {name}: other latents"
    # strength 0.5: the schedule starts in the middle, the kept pixels are still the encoded image
    half = gen(pipe, pos, init_image=photo, inpaint_mask=mask, strength=0.5)
    assert torch.equal(half[..., keep], enc[..., keep]) and not torch.equal(half, a)
    # a white mask is the plain img2img request, a black one returns the encoded image
    white = np.full_like(mask, 255)
    for s in (1.0, 0.5):
        assert torch.equal(gen(pipe, pos, init_image=photo, inpaint_mask=white, strength=s), gen(pipe, pos, init_image=photo, strength=s))
    assert torch.equal(gen(pipe, pos, init_image=photo, inpaint_mask=np.zeros_like(mask)), enc)
    # num_images = 2: both keep the same pixels, the regenerated parts differ (two noise draws)
    two = gen(pipe, pos, init_image=photo, inpaint_mask=mask, num_images=2)
    assert two.shape[0] == 2 and torch.equal(two[0][..., keep], enc[0][..., keep]) and torch.equal(two[1][..., keep], enc[0][..., keep])
    assert not torch.equal(two[0], two[1])
    # through the VAE
    torch.manual_seed(5)
    px = torch.as_tensor(pipe.generate(pos, width=Wpx, height=Hpx, num_steps=6, seed=7, silent=True, output_type="uint8", init_image=photo, inpaint_mask=mask))
    assert px.dtype == torch.uint8 and tuple(px.shape) == (1, Hpx, Wpx, 3)


def test_pipeline_differential(dev, pipe):
    pos, _ = prompts()
    photo, _ = photo_and_mask()
    enc = encoded(pipe, photo)
    ramp = np.tile(np.linspace(0, 255, Wpx).astype(np.uint8)[None], (Hpx, 1))  # left (keep) to right (regenerate)
    ramp[:, :16] = 0
    black = torch.zeros(Hpx // 8, Wpx // 8, dtype=torch.bool, device=enc.device)
    black[:, :2] = True
    binary = gen(pipe, pos, init_image=photo, inpaint_mask=ramp)
    diff = gen(pipe, pos, init_image=photo, inpaint_mask=ramp, inpaint_differential=True)
    assert torch.isfinite(diff).all() and not torch.equal(diff, binary)
    assert torch.equal(diff[..., black], enc[..., black]), "a black column of the change map is not the encoded init image"
    assert torch.equal(binary[..., black], enc[..., black])
    # == Flux.denoise on the pipeline's own pieces with the documented threshold table
    torch.manual_seed(5)
    generator, _ = pipe.set_seed(7)
    x, ts, x0, noise = pipe.preprocess_latent_parts(init_image=torch.from_numpy(photo), height=Hpx, width=Wpx, num_steps=6, generator=generator)
    img, img_ids, vec, txt, txt_ids = map(lambda t: t.contiguous(), pipe.prepare(x, pos))
    m = pipe.prepare_inpaint_mask(ramp, Hpx, Wpx, differential=True)
    thr = [1.0 - (i + 1) / 6 for i in range(6)]
    want = pipe.model.denoise(img, img_ids, txt, txt_ids, vec, ts, guidance=3.5, inpaint_x0=pipe.pack(x0), inpaint_noise=pipe.pack(noise),
                              inpaint_mask=m, inpaint_thresholds=thr)
    assert torch.equal(diff, pipe.unpack(want.float(), Hpx, Wpx))


def test_pipeline_inpaint_compositions(dev, pipe):
    pos, neg = prompts()
    photo, mask = photo_and_mask()
    enc = encoded(pipe, photo)
    keep = keep_of(mask).to(enc.device)
    base = gen(pipe, pos, init_image=photo, inpaint_mask=mask)
    # a Kontext reference: only the noisy rows are blended
    ref = np.random.default_rng(1).integers(0, 256, size=(64, 64, 3), dtype=np.uint8)
    k = gen(pipe, pos, init_image=photo, inpaint_mask=mask, reference_image=ref)
    assert torch.equal(k[..., keep], enc[..., keep]) and not torch.equal(k, base)
    # a negative prompt over the first half of the steps: guided calls and plain calls in one request, differential slices included
    g = gen(pipe, pos, init_image=photo, inpaint_mask=mask, negative_prompt=neg, true_cfg_scale=SCALE, true_cfg_interval=(0, 0.5))
    assert torch.equal(g[..., keep], enc[..., keep]) and not torch.equal(g, base)
    gd = gen(pipe, pos, init_image=photo, inpaint_mask=mask, inpaint_differential=True, negative_prompt=neg, true_cfg_scale=SCALE,
             true_cfg_interval=(0, 0.5))
    assert torch.equal(gd[..., keep], enc[..., keep])
    # step caching
    c = gen(pipe, pos, init_image=photo, inpaint_mask=mask, cache_threshold=1e30, cache_max_hits=1)
    assert torch.equal(c[..., keep], enc[..., keep]) and not torch.equal(c, base)
    # and the request without a mask is unchanged behind all of them
    assert torch.equal(gen(pipe, pos, init_image=photo, inpaint_mask=mask), base)


@pytest.mark.parametrize("in_channels", [128, 384], ids=["control", "fill"])
def test_pipeline_inpaint_on_conditioned_models(dev, in_channels):
    p = tiny_pipeline(dev, in_channels)
    pos, _ = prompts()
    photo, mask = photo_and_mask()
    enc = encoded(p, photo)
    keep = keep_of(mask).to(enc.device)
    if in_channels == 128:
        kw = dict(control_image=np.random.default_rng(2).integers(0, 256, size=(Hpx, Wpx, 3), dtype=np.uint8))
    else:
        kw = dict(mask_image=mask)  # Fill's own conditioning; inpaint_mask is the hard composite on top (strength 1: the encode still runs)
    a = gen(p, pos, init_image=photo, inpaint_mask=mask, **kw)
    assert torch.isfinite(a).all() and torch.equal(a[..., keep], enc[..., keep]), "a kept latent pixel is not the encoded init image"
    plain = gen(p, pos, init_image=photo, **kw)
    assert not torch.equal(a, plain) and not torch.equal(plain[..., keep], enc[..., keep])
    assert torch.equal(gen(p, pos, init_image=photo, inpaint_mask=np.full_like(mask, 255), strength=0.5, **kw), gen(p, pos, init_image=photo, strength=0.5, **kw))


def test_refusals(dev, pipe):
    pos, _ = prompts()
    photo, mask = photo_and_mask()
    kw = dict(width=Wpx, height=Hpx, num_steps=6, seed=7, silent=True, output_type="latent")
    with pytest.raises(ValueError, match="inpaint_mask needs init_image"):
        pipe.generate(pos, inpaint_mask=mask, **kw)
    with pytest.raises(ValueError, match="inpaint_differential needs an inpaint_mask"):
        pipe.generate(pos, init_image=photo, inpaint_differential=True, **kw)
    for bad in (3.5, torch.zeros(Hpx, Wpx), {"mask": mask}):
        with pytest.raises(TypeError, match="inpaint_mask"):
            pipe.generate(pos, init_image=photo, inpaint_mask=bad, **kw)
    # mask_image stays FLUX.1 Fill's: a plain model refuses it as before
    with pytest.raises(ValueError, match="need a FLUX.1 Fill"):
        pipe.generate(pos, init_image=photo, mask_image=mask, **kw)
    # mismatched tensors at denoise, before any device work
    cfg = tiny_config()
    model, _ = build(cfg, None, dev)
    d = to_dev(inputs("plain", cfg.params, 64, 64, 32, 2, seed=2), dev)
    x0, noise, m = iu.make_inpaint(2, d["img"].shape[1], 64, 2, device=dev)
    ts = fo.get_schedule(4, d["img"].shape[1])
    with pytest.raises(ValueError, match="go together"):
        model.denoise(d["img"], d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts, inpaint_x0=x0, inpaint_mask=m)
    with pytest.raises(ValueError, match="inpaint_x0"):
        denoise(model, d, ts, inp=(x0[:1], noise, m))
    with pytest.raises(ValueError, match="inpaint_noise"):
        denoise(model, d, ts, inp=(x0, noise[:, :-1], m))
    with pytest.raises(ValueError, match="inpaint_mask"):
        denoise(model, d, ts, inp=(x0, noise, m[..., :32]))
    with pytest.raises(ValueError, match="inpaint_thresholds"):
        denoise(model, d, ts, inp=(x0, noise, m), thr=[0.5] * 5)
    with pytest.raises(ValueError, match="inpaint_thresholds"):
        model.denoise(d["img"], d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts, inpaint_thresholds=[0.5] * 4)
    assert model._engine is None, "a refused call reached the device"
    # the C entry: a state for another number of images / steps than the call's is refused by the denoise call
    from fluxmi import _lib, ops

    out = denoise(model, d, ts, inp=(x0, noise, m))
    assert torch.isfinite(out).all()
    t_io, tsc, img = C.c_int(0), (C.c_double * len(ts))(*ts), d["img"].clone()
    thr = (C.c_double * 9)(*([0.5] * 9))
    with model._lock:
        _lib.call("fluxmi_engine_set_inpaint", model._engine, ops._p(x0), ops._p(noise), ops._p(m.expand(2, -1, -1).contiguous()), 1, None, 0, ops._stream())
        with pytest.raises(RuntimeError, match="inpainting state holds 1 images"):
            _lib.call("fluxmi_engine_denoise", model._engine, ops._p(img), ops._p(d["txt"]), ops._p(d["y"]), 3.5, tsc, len(ts) - 1, C.byref(t_io), 1, ops._stream())
        _lib.call("fluxmi_engine_set_inpaint", model._engine, ops._p(x0), ops._p(noise), ops._p(m.expand(2, -1, -1).contiguous()), 2, thr, 9, ops._stream())
        with pytest.raises(RuntimeError, match="9 differential thresholds for a call of 4"):
            _lib.call("fluxmi_engine_denoise", model._engine, ops._p(img), ops._p(d["txt"]), ops._p(d["y"]), 3.5, tsc, len(ts) - 1, C.byref(t_io), 1, ops._stream())
        with pytest.raises(RuntimeError, match="engine_set_inpaint: batch 3"):
            _lib.call("fluxmi_engine_set_inpaint", model._engine, ops._p(x0), ops._p(noise), ops._p(m), 3, None, 0, ops._stream())
        with pytest.raises(RuntimeError, match="go together"):
            _lib.call("fluxmi_engine_set_inpaint", model._engine, ops._p(x0), None, ops._p(m), 2, None, 0, ops._stream())
        _lib.call("fluxmi_engine_set_inpaint", model._engine, None, None, None, 0, None, 0, ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(img, d["img"])
    # n_steps = 0 with a (zero-entry) threshold table: nothing to do, the latents come back
    zero = denoise(model, d, ts[:1], inp=(x0, noise, m), thr=[])
    assert torch.equal(zero, d["img"])
