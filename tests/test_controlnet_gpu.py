"""FLUX ControlNet on the GPU: the engine runs the net's block stack and the main trunk inside one step (fluxmi_engine_attach_controlnet) and
hands the per-block residuals over with fluxmi_add_scaled.  The reference is tests/controlnet_ref.py, a restatement of diffusers'
FluxControlNetModel / FluxTransformer2DModel composed from the oracle's blocks (parity with diffusers itself is unpinned).

Tiny geometry of tests/test_kontext_gpu.py (hidden 256, 2 heads, ctx 128, vec 64); the main model has 3 double and 4 single blocks, so a net of
2 + 2 blocks feeds them at an interval of 2.  Gates are that file's: rel-L2 <= 1e-2 (bf16 flow), <= 6e-2 against the fp8 oracle and, at calls 0, 7
and 14, distance to the bf16 oracle <= 1.25 x the fp8 oracle's own.  tests/test_controlnet_cpu.py shows that the synthetic projections move the
oracle's output by >= 0.1 rel-L2, so none of this passes with the net ignored."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

import controlnet_ref as cr
import flux_oracle as fo
import knob_contract as kc
from test_kontext_gpu import QUANTS, rel_l2, to_dev

pytestmark = pytest.mark.gpu

NETS = {"2+2": (2, 2, 0), "union": (2, 1, 3), "2+0": (2, 0, 0)}  # double, single, modes
GATE = {"bf16": 1e-2, "fp8": 6e-2, "fp8_emb": 6e-2}


def tiny_config():
    import util

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    p = cfg.params
    p.hidden_size, p.num_heads, p.depth, p.depth_single_blocks, p.context_in_dim, p.vec_in_dim = 256, 2, 3, 4, 128, 64
    return cfg


def quantise(m, quant, dev):
    from float8_quantize import quantize_flow_transformer_and_dispatch_float8

    m.to(dev)
    if quant is not None:
        quantize_flow_transformer_and_dispatch_float8(m, dev, flow_dtype=torch.bfloat16, swap_linears_with_cublaslinear=False,
                                                      quantize_modulation=quant["modulation"], quantize_flow_embedder_layers=quant["embedders"])
    return m


def build_main(cfg, quant, dev, seed=0):
    import util
    from fluxmi import synth

    sd = synth.make_state_dict(cfg.params, seed=seed)
    return quantise(util.load_flow_model(cfg, {k: v.clone() for k, v in sd.items()}), quant, dev), sd


def build_net(cfg, spec, quant, dev, seed=0, zero=False):
    from fluxmi import synth
    from modules.controlnet import FluxControlNet

    sd = synth.make_controlnet_state_dict(cfg.params, *spec, seed=seed)
    if zero:
        for k in sd:
            if k.startswith(("controlnet_blocks", "controlnet_single_blocks")):
                sd[k] = torch.zeros_like(sd[k])
    return quantise(FluxControlNet.from_state_dict(cfg, {k: v.clone() for k, v in sd.items()}), quant, dev), sd


def oracles(cfg, sd, net_sd, quant):
    params = fo.FluxParams(**cfg.params.model_dump())
    return fo.FluxOracle({k: v.clone() for k, v in sd.items()}, params, quantize=quant), cr.make_net_oracle(net_sd, params, quantize=quant)


def inputs(params, H, W, Lt, B, seed):
    from fluxmi import synth

    inp = synth.make_inputs(params, H, W, Lt, batch=B, seed=seed, real_tokens=8)
    g = torch.Generator().manual_seed(900 + seed)
    inp["cond"] = torch.randn(B, inp["img"].shape[1], params.in_channels, generator=g).to(torch.bfloat16)
    return inp


def call_of(net, d, scale=1.0, mode=None):
    from modules.controlnet import ControlNetCall

    return ControlNetCall(net, d["cond"], scale, mode)


def den(model, d, ts, cn=None, use_graph=True, img=None, **kw):
    return model.denoise(d["img"] if img is None else img, d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts, guidance=3.5, use_graph=use_graph,
                         controlnet=cn, **kw)


def ref_den(main, net, inp, ts, img=None, **kw):
    return cr.denoise(main, net, inp["img"] if img is None else img, inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], ts, cond=inp["cond"], **kw)


def calibrate(model, d, ts16, cn=None):
    """14 eager steps: 13 calibrating calls of every F8Linear of the main model (and of the attached net)"""
    lat = den(model, d, ts16[:15], cn=cn, use_graph=False)
    assert model.calibration_state()[0] is not False and (cn is None or cn.net.calibration_state()[0] is not False)
    return lat


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 4099])
def test_add_scaled_kernel_bit_exact(dev, n):
    from fluxmi import _lib, ops

    g = torch.Generator().manual_seed(n)
    B, pad = 3, 13
    for s in (0.0, 0.7, 1.0, -1.5):
        for xs, rs in ((n + pad, n), (n + 8 - n % 8 + 8, n + 8 - n % 8)):  # an odd x stride (element accesses) / 16-byte aligned strides
            xbuf = torch.randn(B, xs, generator=g).to(torch.bfloat16).to(dev)
            rbuf = torch.randn(B, rs, generator=g).to(torch.bfloat16).to(dev)
            before = xbuf.clone()
            x, r = xbuf[:, :n], rbuf[:, :n]
            want = x + r * s  # bf16 tensors, python scalar: bf16(x + bf16(r * fp32(s)))
            assert want.dtype == torch.bfloat16
            sd = torch.tensor([s], dtype=torch.float32, device=dev)
            _lib.call("fluxmi_add_scaled", ops._p(x), xs, ops._p(r), rs, ops._p(sd), B, n, ops._stream())
            torch.cuda.synchronize()
            assert torch.equal(xbuf[:, :n], want), f"n={n} s={s} strides {xs}/{rs}: rel-L2 {rel_l2(xbuf[:, :n], want):.3e}"
            assert torch.equal(xbuf[:, n:], before[:, n:]), f"n={n} s={s}: wrote past a sample's n elements"
            if s == 0.0:
                assert torch.equal(xbuf, before)
    # the host wrapper: a float scale, dense tensors, more than one workgroup per sample
    x = torch.randn(2, 5, 4099, generator=g).to(torch.bfloat16).to(dev)
    r = torch.randn(2, 5, 4099, generator=g).to(torch.bfloat16).to(dev)
    want = x + r * 0.3
    assert torch.equal(ops.add_scaled(x, r, 0.3), want)
    with pytest.raises(RuntimeError, match="strides"):
        _lib.call("fluxmi_add_scaled", ops._p(x), 8, ops._p(r), 8, ops._p(torch.ones(1, device=dev)), 2, 16, ops._stream())


# ---- 2. zeroed projections: the request without a net, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("qname", ["bf16", "fp8"])
def test_zeroed_projections_change_nothing(dev, qname):
    cfg = tiny_config()
    model, _ = build_main(cfg, QUANTS[qname], dev)
    net, _ = build_net(cfg, NETS["union"], QUANTS[qname], dev, zero=True)
    B, H, W, Lt = 2, 64, 64, 32
    d = to_dev(inputs(cfg.params, H, W, Lt, B, seed=5), dev)
    cn = call_of(net, d, 0.7, mode=1)
    ts = fo.get_schedule(16, 16)
    lat = calibrate(model, d, ts, cn=cn)
    ts2 = ts[:5]
    plain = den(model, d, ts2, img=lat)
    assert torch.equal(den(model, d, ts2, cn=cn, img=lat), plain)
    assert torch.equal(den(model, d, ts2, cn=cn, img=lat, use_graph=False), plain)
    t = torch.full((B,), 0.5, dtype=torch.bfloat16, device=dev)
    g = torch.full((B,), 3.5, dtype=torch.bfloat16, device=dev)
    args = (lat, d["img_ids"], d["txt"], d["txt_ids"], t, d["y"], g)
    assert torch.equal(model(*args, controlnet=cn), model(*args))


# ---- 3. forward through calibration against the composed oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("qname", list(QUANTS))
@pytest.mark.parametrize("shape", [(64, 64, 32, 2, "2+2", None), (48, 80, 40, 1, "union", 1), (64, 64, 32, 1, "2+0", None)])
def test_forward_matches_oracle_through_calibration(dev, qname, shape):
    H, W, Lt, B, nname, mode = shape
    cfg = tiny_config()
    model, sd = build_main(cfg, QUANTS[qname], dev)
    net, net_sd = build_net(cfg, NETS[nname], QUANTS[qname], dev)
    o_main, o_net = oracles(cfg, sd, net_sd, QUANTS[qname])
    b_main, b_net = oracles(cfg, sd, net_sd, None)
    inp = inputs(cfg.params, H, W, Lt, B, seed=3)
    d = to_dev(inp, dev)
    Li = inp["img"].shape[1]
    assert Li == (15 if nname == "union" else 16)
    cn = call_of(net, d, 0.7, mode)
    worst = 0.0
    for step in range(15):
        t = torch.full((B,), 1.0 - 0.06 * step, dtype=torch.bfloat16)
        g = torch.full((B,), 3.5, dtype=torch.bfloat16)
        args = (inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], t, inp["y"], g)
        ref = cr.forward(o_main, o_net, *args, cond=inp["cond"], mode=mode, scale=0.7)
        got = model(d["img"], d["img_ids"], d["txt"], d["txt_ids"], t.to(dev), d["y"], g.to(dev), controlnet=cn)
        assert got.shape == (B, Li, 64) and torch.isfinite(got).all()
        e = rel_l2(got, ref)
        worst = max(worst, e)
        print(f"[controlnet {qname} {nname}] call {step}: rel-L2 {e:.3e}")
        assert e <= GATE[qname], f"{qname} {nname} call {step}: rel-L2 {e:.3e}"
        if QUANTS[qname] is not None and step in (0, 7, 14):
            rb = cr.forward(b_main, b_net, *args, cond=inp["cond"], mode=mode, scale=0.7)
            d_ref, d_got = rel_l2(ref, rb), rel_l2(got, rb)
            print(f"[controlnet {qname} {nname}] call {step}: vs bf16 flow {d_got:.3e}, the fp8 oracle's own {d_ref:.3e}")
            assert d_got <= 1.25 * d_ref, f"{qname} {nname} call {step}: vs bf16 flow {d_got:.3e} > 1.25 x {d_ref:.3e}"
    if QUANTS[qname] is not None:
        assert model.calibration_state()[0] and net.calibration_state()[0]
        for mod, orc, what in ((model, o_main, "main"), (net, o_net, "net")):
            names = [n for n, m in orc.lin.items() if isinstance(m, fo.F8LinearState)]
            exact = 0
            for n in names:
                so, sg = orc.lin[n].input_scale.item(), mod.get_submodule(n).input_scale.item()
                assert abs(sg - so) <= 0.30 * so, f"{what} {n}: input_scale {sg} vs oracle {so}"
                exact += int(sg == so)
            assert exact >= 0.3 * len(names), f"{what}: only {exact}/{len(names)} input scales bit-identical"
    print(f"[controlnet {qname} {shape}] worst rel-L2 over 15 calls: {worst:.3e}")


# ---- 4. denoise against the oracle loop; graph == eager; two scales back to back --------------------------------------------------------------
@pytest.mark.parametrize("qname", ["bf16", "fp8"])
def test_denoise_matches_oracle_and_graph_equals_eager(dev, qname):
    cfg = tiny_config()
    model, sd = build_main(cfg, QUANTS[qname], dev)
    net, net_sd = build_net(cfg, NETS["union"], QUANTS[qname], dev)
    o_main, o_net = oracles(cfg, sd, net_sd, QUANTS[qname])
    B, H, W, Lt = 1, 64, 64, 32
    inp = inputs(cfg.params, H, W, Lt, B, seed=7)
    d = to_dev(inp, dev)
    ts = fo.get_schedule(16, 16)
    ref = ref_den(o_main, o_net, inp, ts, mode=2, scale=0.8)
    got = den(model, d, ts, cn=call_of(net, d, 0.8, 2))
    e = rel_l2(got, ref)
    print(f"[controlnet {qname}] latents after 16 steps: rel-L2 {e:.3e}")
    assert got.shape == inp["img"].shape and e <= GATE[qname]
    assert model.calibration_state()[0] is not False and net.calibration_state()[0] is not False
    # frozen now: two requests at scales 0.4 and 1.0 back to back, each against the oracle at ITS scale, graph == eager
    ts2 = ts[:5]
    for s in (0.4, 1.0):
        cn = call_of(net, d, s, 2)
        a = den(model, d, ts2, cn=cn)
        b = den(model, d, ts2, cn=cn, use_graph=False)
        assert torch.equal(a, b), f"scale {s}: graph vs eager rel-L2 {rel_l2(a, b):.3e}"
        r = ref_den(o_main, o_net, inp, ts2, mode=2, scale=s)
        e = rel_l2(a, r)
        print(f"[controlnet {qname}] scale {s}: rel-L2 {e:.3e}")
        assert e <= GATE[qname], f"scale {s}: rel-L2 {e:.3e}"
    assert not torch.equal(den(model, d, ts2, cn=call_of(net, d, 0.4, 2)), a), "the scale does not reach the latents"
    # the python loop over Flux.forward is the same request
    cn = call_of(net, d, 0.4, 2)
    c = d["img"].clone()
    g = torch.full((B,), 3.5, dtype=torch.bfloat16, device=dev)
    for t_curr, t_prev in zip(ts2[:-1], ts2[1:]):
        tv = torch.full((B,), t_curr, dtype=torch.bfloat16, device=dev)
        c = c + (t_prev - t_curr) * model(c, d["img_ids"], d["txt"], d["txt_ids"], tv, d["y"], g, controlnet=cn)
    assert torch.equal(den(model, d, ts2, cn=cn), c)


# ---- 5. step interval ----------------------------------------------------------------------------------------------------------------------
def test_interval_is_consecutive_denoise_calls(dev):
    from modules.controlnet import control_steps

    cfg = tiny_config()
    model, _ = build_main(cfg, None, dev)
    net, _ = build_net(cfg, NETS["2+2"], None, dev)
    d = to_dev(inputs(cfg.params, 64, 64, 32, 2, seed=9), dev)
    ts = fo.get_schedule(4, 16)
    cn = call_of(net, d, 0.9)

    def request(start, end):
        keep, x, i = control_steps(4, start, end), d["img"], 0
        while i < 4:
            j = i
            while j < 4 and keep[j] == keep[i]:
                j += 1
            x = den(model, d, ts[i:j + 1], cn=cn if keep[i] else None, img=x)
            i = j
        return x

    plain = den(model, d, ts)
    assert torch.equal(request(0.0, 0.0), plain)
    half = request(0.0, 0.5)
    assert torch.equal(half, den(model, d, ts[2:], img=den(model, d, ts[:3], cn=cn)))
    full = request(0.0, 1.0)
    assert torch.equal(full, den(model, d, ts, cn=cn))
    assert not torch.equal(half, plain) and not torch.equal(half, full)


def test_a_replaced_net_never_replays_the_old_nets_graph(dev):
    """A captured step holds the attached net's workspace and weights.  The graph is keyed on a generation number no other net of the process
    ever has, not on the net's address: a net created after another was destroyed (the allocator may hand its address out again) re-captures,
    and its latents are those of a fresh engine pair."""
    cfg = tiny_config()
    model, _ = build_main(cfg, None, dev)
    d = to_dev(inputs(cfg.params, 64, 64, 32, 2, seed=19), dev)
    ts = fo.get_schedule(4, 16)
    want = {}
    for seed in (0, 1, 2):
        fresh, _ = build_main(cfg, None, dev)
        net, _ = build_net(cfg, NETS["2+2"], None, dev, seed=seed)
        want[seed] = den(fresh, d, ts, cn=call_of(net, d, 0.9))
        net._invalidate_engine()
        fresh._invalidate_engine()
    assert not torch.equal(want[0], want[1]) and not torch.equal(want[1], want[2])
    for seed in (0, 1, 2, 1):
        net, _ = build_net(cfg, NETS["2+2"], None, dev, seed=seed)
        got = den(model, d, ts, cn=call_of(net, d, 0.9))  # a graph-replayed request on the SAME main engine, no plain request in between
        assert torch.equal(got, want[seed]), f"net {seed} behind another net: rel-L2 {rel_l2(got, want[seed]):.3e}"
        assert torch.equal(den(model, d, ts, cn=call_of(net, d, 0.9)), got)
        net._invalidate_engine()  # the net's engine is destroyed while the main engine still holds the graph captured with it
        del net


# ---- 6. a net loaded onto a calibrated model -----------------------------------------------------------------------------------------------
def test_net_loaded_after_the_main_model_is_frozen(dev):
    cfg = tiny_config()
    q = QUANTS["fp8"]
    model, sd = build_main(cfg, q, dev)
    net, net_sd = build_net(cfg, NETS["2+2"], q, dev)
    o_main, o_net = oracles(cfg, sd, net_sd, q)
    B = 2
    inp = inputs(cfg.params, 64, 64, 32, B, seed=11)
    d = to_dev(inp, dev)
    ts = fo.get_schedule(16, 16)
    lat = calibrate(model, d, ts)                      # the main model alone: 13 trials
    o_lat = cr.denoise(o_main, None, inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], ts[:15])
    assert model.calibration_state() == (True, 12) and net.calibration_state() == (False, 0)
    scales = {n: m.input_scale.item() for n, m in model.named_modules() if hasattr(m, "input_scale")}
    cn = call_of(net, d, 0.8)
    got = den(model, d, ts, cn=cn)                     # the net calibrates on ITS counter (13 eager steps), the last 3 steps replay a graph
    assert net.calibration_state() == (True, 12) and model.calibration_state() == (True, 12)
    assert scales == {n: m.input_scale.item() for n, m in model.named_modules() if hasattr(m, "input_scale")}, "the frozen main model's scales moved"
    ref = ref_den(o_main, o_net, inp, ts, scale=0.8)
    e = rel_l2(got, ref)
    print(f"[controlnet on a frozen model] 16 steps: rel-L2 {e:.3e}; plain latents vs oracle {rel_l2(lat, o_lat):.3e}")
    assert e <= GATE["fp8"]
    ms, steps = C.c_float(0), C.c_int(0)
    from fluxmi import _lib

    _lib.call("fluxmi_engine_last_timing", model._engine, C.byref(ms), C.byref(steps))
    assert steps.value == 2, f"{steps.value} graph-replayed steps behind the warm step (16 steps: 13 calibrating, 1 warm, 2 replayed)"
    a = den(model, d, ts[:7], cn=cn)
    _lib.call("fluxmi_engine_last_timing", model._engine, C.byref(ms), C.byref(steps))
    assert steps.value == 6, "a request on two frozen nets is not graph-replayed from its first step"
    assert torch.equal(a, den(model, d, ts[:7], cn=cn, use_graph=False))
    e = rel_l2(a, ref_den(o_main, o_net, inp, ts[:7], scale=0.8))
    print(f"[controlnet on a frozen model] frozen request: rel-L2 {e:.3e}")
    assert e <= GATE["fp8"]


# ---- 7. negative prompt: both branches are controlled ------------------------------------------------------------------------------------------
def oracle_guided(main, net, inp, ts, scale, cfg_scale, mode=None):
    from test_cfg_gpu import dup

    x = inp["img"]
    B = x.shape[0]
    g = torch.full((2 * B,), 3.5, dtype=main.dtype)
    txt, y = torch.cat((inp["txt"], inp["neg_txt"]), 0), torch.cat((inp["y"], inp["neg_y"]), 0)
    for t_curr, t_prev in zip(ts[:-1], ts[1:]):
        tv = torch.full((2 * B,), t_curr, dtype=main.dtype)
        pred = cr.forward(main, net, dup(x), dup(inp["img_ids"]), txt, dup(inp["txt_ids"]), tv, y, g, cond=dup(inp["cond"]), mode=mode, scale=scale)
        c, u = pred[:B], pred[B:]
        x = x + (t_prev - t_curr) * (u + cfg_scale * (c - u))
    return x


def test_negative_prompt_controls_both_branches(dev, monkeypatch):
    """tests/test_cfg_gpu.py's gates: bf16 flow rel-L2 <= max(1e-2, 1.75 x floor), floor = the oracle's own movement when its SDPA is replaced
    by fo.attention_exact; fp8 flow: distance to the bf16 oracle <= 1.25 x the fp8 oracle's own."""
    from fluxmi import synth

    cfg = tiny_config()
    B, n, S = 1, 16, 3.5
    ts = fo.get_schedule(n, 16)
    inp = inputs(cfg.params, 64, 64, 32, B, seed=13)
    neg = synth.make_inputs(cfg.params, 64, 64, 32, batch=B, seed=113, real_tokens=4)
    inp["neg_txt"], inp["neg_y"] = neg["txt"], neg["y"]
    d = to_dev(inp, dev)
    ref = {}
    for qname in ("bf16", "fp8"):
        model, sd = build_main(cfg, QUANTS[qname], dev)
        net, net_sd = build_net(cfg, NETS["2+2"], QUANTS[qname], dev)
        if not ref:
            ref["o16"] = oracle_guided(*oracles(cfg, sd, net_sd, None), inp, ts, 0.8, S)
            with monkeypatch.context() as mp:
                mp.setattr(fo, "attention", fo.attention_exact)
                ref["floor"] = rel_l2(oracle_guided(*oracles(cfg, sd, net_sd, None), inp, ts, 0.8, S), ref["o16"])
        got = den(model, d, ts, cn=call_of(net, d, 0.8), neg_txt=d["neg_txt"], neg_y=d["neg_y"], cfg_scale=S)
        assert got.shape == inp["img"].shape and torch.isfinite(got).all()
        e16 = rel_l2(got, ref["o16"])
        if qname == "bf16":
            gate = max(1e-2, 1.75 * ref["floor"])
            print(f"[controlnet cfg bf16] engine vs oracle {e16:.3e}; floor {ref['floor']:.3e}; gate {gate:.3e}")
            assert e16 <= gate
            one = den(model, d, ts, cn=call_of(net, d, 0.8))
            assert not torch.equal(one, got), "the negative branch has no effect"
        else:
            yard = rel_l2(oracle_guided(*oracles(cfg, sd, net_sd, QUANTS[qname]), inp, ts, 0.8, S), ref["o16"])
            print(f"[controlnet cfg fp8] engine vs oracle-bf16 {e16:.3e}; yardstick {yard:.3e}; ratio {e16 / yard:.3f} (gate 1.25)")
            assert e16 <= 1.25 * yard
            ts2 = ts[:5]
            kw = dict(cn=call_of(net, d, 0.8), neg_txt=d["neg_txt"], neg_y=d["neg_y"], cfg_scale=S)
            assert torch.equal(den(model, d, ts2, **kw), den(model, d, ts2, use_graph=False, **kw))


# ---- 8. inpainting, knobs, detach ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qname", ["fp8", "bf16"])
def test_inpaint_knobs_and_detach(dev, qname):
    from fluxmi import _lib

    cfg = tiny_config()
    model, _ = build_main(cfg, QUANTS[qname], dev)
    net, _ = build_net(cfg, NETS["union"], QUANTS[qname], dev)
    B = 2
    d = to_dev(inputs(cfg.params, 64, 64, 32, B, seed=15), dev)
    cn = call_of(net, d, 0.8, 0)
    ts = fo.get_schedule(16, 16)
    before = den(model, d, ts[:5]) if QUANTS[qname] is None else None
    lat = calibrate(model, d, ts, cn=cn)
    ts2 = ts[:5]
    plain = den(model, d, ts2, img=lat)
    a = den(model, d, ts2, cn=cn, img=lat)
    assert not torch.equal(a, plain)
    # every knob set the contract table lists as bit-identical for this flow leaves the controlled latents bit-identical
    flow = "bf16" if QUANTS[qname] is None else "fp8"
    ran = 0
    for name, v, c in kc.sweep(flow):
        if c.kind != "bit":
            continue
        knobs = kc.knobs_of(name, v, c)
        with _lib.tuning(**knobs):
            a3 = den(model, d, ts2, cn=cn, img=lat)
        assert torch.equal(a, a3), f"controlled latents change under tuning {knobs}: rel-L2 {rel_l2(a3, a):.3e}"
        ran += 1
    assert ran >= 8
    # masked-latent inpainting composes: the kept elements of a schedule that ends at 0 are the init latent, bit for bit
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(B, 16, 64, generator=g).to(torch.bfloat16).to(dev)
    noise = torch.randn(B, 16, 64, generator=g).to(torch.bfloat16).to(dev)
    mask = (torch.rand(B, 16, 1, generator=g) < 0.5).to(torch.bfloat16).expand(B, 16, 64).contiguous().to(dev)
    ts3 = ts[-5:]
    assert ts3[-1] == 0.0
    ikw = dict(inpaint_x0=x0, inpaint_noise=noise, inpaint_mask=mask)
    m = den(model, d, ts3, cn=cn, img=lat, **ikw)
    assert torch.equal(m[mask == 0], x0[mask == 0]) and not torch.equal(m[mask == 1], x0[mask == 1])
    assert torch.equal(m, den(model, d, ts3, cn=cn, img=lat, use_graph=False, **ikw))
    assert not torch.equal(m, den(model, d, ts3, img=lat, **ikw)), "the ControlNet has no effect on a masked request"
    # detached again: the plain request is what it was, and a controlled one behind it what IT was
    assert torch.equal(den(model, d, ts2, img=lat), plain)
    assert torch.equal(den(model, d, ts2, cn=cn, img=lat), a)
    if before is not None:
        assert torch.equal(den(model, d, ts[:5]), before), "a plain request differs from the one made before a net was ever attached"


# ---- 9. engine refusals --------------------------------------------------------------------------------------------------------------------
def test_engine_refusals(dev):
    import util
    from fluxmi import _lib, ops, synth
    from modules.controlnet import FluxControlNet

    cfg = tiny_config()
    model, _ = build_main(cfg, None, dev)
    net, _ = build_net(cfg, NETS["2+0"], None, dev)
    union, _ = build_net(cfg, NETS["union"], None, dev)
    B = 2
    d = to_dev(inputs(cfg.params, 64, 64, 32, B, seed=17), dev)
    Li, Lt = d["img"].shape[1], d["txt"].shape[1]
    cond = d["cond"].contiguous()

    def prepared(m, Lc=0, img=None, ids=None):
        m._ensure_engine(dev)
        img = d["img"] if img is None else img
        m._prepare(img, d["img_ids"] if ids is None else ids, d["txt_ids"], d["txt"], Lc)

    prepared(model)
    for n in (net, union):
        n._ensure_engine(dev)
    attach = lambda m, n, c=cond, batch=B, mode=-1: _lib.call("fluxmi_engine_attach_controlnet", m._engine, n._engine, ops._p(c), batch, mode, 1.0, 0,
                                                             ops._stream())
    attach(model, net)
    attach(model, net, batch=1)  # half the batch: a guided request's cond
    with pytest.raises(RuntimeError, match="prepared batch"):
        attach(model, net, batch=3)
    with pytest.raises(RuntimeError, match="without a mode embedding"):
        attach(model, net, mode=0)
    for mode in (-1, 3):
        with pytest.raises(RuntimeError, match="control mode"):
            attach(model, union, mode=mode)
    attach(model, union, mode=2)
    # a ControlNet handle is not a main engine
    with pytest.raises(RuntimeError, match="ControlNet engine"):
        _lib.call("fluxmi_engine_prepare", net._engine, B, Li, Lt, ops._p(d["img_ids"]), ops._p(d["txt_ids"]), ops._stream())
    with pytest.raises(RuntimeError, match="main engine"):
        attach(net, union, mode=2)
    with pytest.raises(RuntimeError, match="not a ControlNet"):
        _lib.call("fluxmi_engine_attach_controlnet", model._engine, model._engine, ops._p(cond), B, -1, 1.0, 0, ops._stream())
    # attention-group table, step caching
    table = torch.full((B, Lt + Li), 1 << 16, dtype=torch.int32, device=dev)  # key group 0, admits group 0
    _lib.call("fluxmi_engine_set_attn_groups", model._engine, ops._p(table), ops._stream())
    with pytest.raises(RuntimeError, match="attention table"):
        attach(model, net)
    _lib.call("fluxmi_engine_set_attn_groups", model._engine, None, ops._stream())
    _lib.call("fluxmi_engine_set_step_cache", model._engine, 0.1, 0)
    with pytest.raises(RuntimeError, match="step caching"):
        attach(model, net)
    _lib.call("fluxmi_engine_set_step_cache", model._engine, 0.0, 0)
    attach(model, net)
    _lib.call("fluxmi_engine_set_step_cache", model._engine, 0.1, 0)  # switched on behind the attach: the denoise call refuses
    img = d["img"].clone()
    ts = (C.c_double * 3)(1.0, 0.5, 0.0)
    t_io = C.c_int(0)
    with pytest.raises(RuntimeError, match="step caching"):
        _lib.call("fluxmi_engine_denoise", model._engine, ops._p(img), ops._p(d["txt"]), ops._p(d["y"]), 3.5, ts, 2, C.byref(t_io), 1, ops._stream())
    _lib.call("fluxmi_engine_set_step_cache", model._engine, 0.0, 0)
    _lib.call("fluxmi_engine_attach_controlnet", model._engine, None, None, 0, -1, 1.0, 0, ops._stream())
    # Kontext reference rows
    prepared(model, Lc=4, img=torch.cat((d["img"], d["img"][:, :4]), 1), ids=torch.cat((d["img_ids"], d["img_ids"][:, :4]), 1))
    with pytest.raises(RuntimeError, match="Kontext reference rows"):
        attach(model, net)
    # another geometry; a channel-conditioned main model
    wcfg = tiny_config()
    wcfg.params.hidden_size, wcfg.params.num_heads = 384, 3
    wide, _ = build_net(wcfg, NETS["2+0"], None, dev)
    wide._ensure_engine(dev)
    prepared(model)
    with pytest.raises(RuntimeError, match="differ from the main model"):
        attach(model, wide)
    fcfg = tiny_config()
    fcfg.params.in_channels, fcfg.params.out_channels = 128, 64
    fill = util.load_flow_model(fcfg, synth.make_state_dict(fcfg.params, seed=0)).to(dev)
    ncfg = tiny_config()
    ncfg.params.in_channels = 128
    net128 = FluxControlNet.from_state_dict(ncfg, synth.make_controlnet_state_dict(ncfg.params, 2, 0, seed=0)).to(dev)
    net128._ensure_engine(dev)
    img128 = torch.cat((d["img"], d["img"]), 2).contiguous()
    prepared(fill, img=img128)
    with pytest.raises(RuntimeError, match="channel-conditioned"):
        attach(fill, net128, c=img128)
    # a net with a guidance embedder on a main model without one; the phase hook with a net attached
    import util as _util

    scfg = tiny_config()
    scfg.params.guidance_embed = False
    plain_main = _util.load_flow_model(scfg, synth.make_state_dict(scfg.params, seed=0)).to(dev)
    prepared(plain_main)
    with pytest.raises(RuntimeError, match="guidance embedder"):
        attach(plain_main, net)
    prepared(model)
    attach(model, net)
    with pytest.raises(RuntimeError, match="ControlNet is attached"):
        _lib.call("fluxmi_engine_run_phase", model._engine, 2, 0, 3, -1, ops._stream())
    _lib.call("fluxmi_engine_attach_controlnet", model._engine, None, None, 0, -1, 1.0, 0, ops._stream())
    # the controlnet_* projections must stay bf16
    bad, _ = build_net(cfg, NETS["2+0"], None, dev)
    from float8_quantize import F8Linear

    bad.controlnet_blocks[0] = F8Linear.from_linear(bad.controlnet_blocks[0])
    with pytest.raises(ValueError, match="stay bf16"):
        bad._ensure_engine(dev)


# ---- 10. the pipeline, end to end through the tiny VAE ---------------------------------------------------------------------------------------
def test_pipeline_controlnet_through_vae(dev):
    import util
    from PIL import Image

    from flux_pipeline import FluxPipeline
    from fluxmi import synth
    from modules.autoencoder import AutoEncoder, AutoEncoderParams

    cfg = tiny_config()
    cfg.text_enc_max_length = 32
    cfg.ae_device = str(dev)
    cfg.ae_params = AutoEncoderParams(resolution=32, in_channels=3, ch=32, out_ch=3, ch_mult=[1, 2, 2, 2], num_res_blocks=1, z_channels=16,
                                      scale_factor=0.3611, shift_factor=0.1159)
    torch.manual_seed(0)
    ae_sd = {k: v.clone() for k, v in AutoEncoder(cfg.ae_params).state_dict().items()}
    pipe = FluxPipeline.load_pipeline_from_config(cfg, state_dict=synth.make_state_dict(cfg.params, seed=0), ae_state_dict=ae_sd)
    assert pipe.controlnet is None
    pipe.controlnet = util.load_controlnet(cfg, device=dev, state_dict=synth.make_controlnet_state_dict(cfg.params, 2, 1, 3, seed=0))
    pipe.compile()
    assert pipe.model.calibration_state()[0] and pipe.controlnet.calibration_state()[0], "compile() did not calibrate both nets"
    g = torch.Generator().manual_seed(1)
    prompt = {"txt": 0.1 * torch.randn(1, 32, 128, generator=g), "vec": torch.randn(1, 64, generator=g)}
    edges = np.random.default_rng(0).integers(0, 256, size=(90, 60, 3), dtype=np.uint8)
    kw = dict(width=64, height=96, num_steps=6, seed=7, silent=True)

    def gen(**k):
        torch.manual_seed(5)  # the VAE encoder's Gaussian sample
        return pipe.generate(prompt, **kw, **k)

    buf = gen(controlnet_image=edges, control_mode=1)
    assert isinstance(buf, io.BytesIO) and Image.open(buf).size == (64, 96)
    assert gen(controlnet_image=edges, control_mode=1).getvalue() == buf.getvalue(), "same seed, different bytes"
    assert gen(controlnet_image=Image.fromarray(edges), control_mode=1).getvalue() == buf.getvalue()
    plain = gen(output_type="latent")
    lat = gen(controlnet_image=edges, control_mode=1, controlnet_conditioning_scale=0.7, output_type="latent")
    assert torch.isfinite(lat).all() and not torch.equal(lat, plain)
    assert not torch.equal(gen(controlnet_image=edges, control_mode=2, controlnet_conditioning_scale=0.7, output_type="latent"), lat)
    assert torch.equal(gen(controlnet_image=edges, control_mode=1, control_guidance_end=0.0, output_type="latent"), plain)
    assert torch.equal(gen(controlnet_image=edges, control_mode=1, controlnet_conditioning_scale=0.0, output_type="latent"), plain)
    part = gen(controlnet_image=edges, control_mode=1, controlnet_conditioning_scale=0.7, control_guidance_start=0.0, control_guidance_end=0.5,
               output_type="latent")
    assert not torch.equal(part, lat) and not torch.equal(part, plain)
    # == Flux.denoise on the pipeline's own pieces (the cond's VAE sample is drawn after the noise)
    from modules.controlnet import ControlNetCall

    torch.manual_seed(5)
    generator, _ = pipe.set_seed(7)
    noise, ts = pipe.preprocess_latent(height=96, width=64, num_steps=6, generator=generator, num_images=1)
    img, img_ids, vec, txt, txt_ids = map(lambda x: x.contiguous(), pipe.prepare(noise, prompt))
    cond = pipe.prepare_controlnet_conditioning(edges, 96, 64, num_images=1, generator=generator)
    assert cond.shape == (1, 24, 64) and cond.dtype == torch.bfloat16
    want = pipe.model.denoise(img, img_ids, txt, txt_ids, vec, ts, guidance=3.5, controlnet=ControlNetCall(pipe.controlnet, cond, 0.7, 1))
    assert torch.equal(lat, pipe.unpack(want.float(), 96, 64))
    # control_guidance_end = 0.5 of 6 steps: generate cuts the schedule into a controlled call on steps 0..2 and a plain one on steps 3..5
    first = pipe.model.denoise(img, img_ids, txt, txt_ids, vec, ts[:4], guidance=3.5, controlnet=ControlNetCall(pipe.controlnet, cond, 0.7, 1))
    both = pipe.model.denoise(first, img_ids, txt, txt_ids, vec, ts[3:], guidance=3.5)
    assert torch.equal(part, pipe.unpack(both.float(), 96, 64)), "generate(control_guidance_end=0.5) is not the two explicit denoise calls"
    late = gen(controlnet_image=edges, control_mode=1, controlnet_conditioning_scale=0.7, control_guidance_start=0.5, output_type="latent")
    first = pipe.model.denoise(img, img_ids, txt, txt_ids, vec, ts[:4], guidance=3.5)
    both = pipe.model.denoise(first, img_ids, txt, txt_ids, vec, ts[3:], guidance=3.5, controlnet=ControlNetCall(pipe.controlnet, cond, 0.7, 1))
    assert torch.equal(late, pipe.unpack(both.float(), 96, 64)), "generate(control_guidance_start=0.5) is not the two explicit denoise calls"
    # compositions: two images, img2img, a negative prompt, an inpainting mask
    two = gen(controlnet_image=edges, control_mode=1, num_images=2)
    assert Image.open(two).size == (64, 2 * 96)
    photo = np.random.default_rng(1).integers(0, 256, size=(96, 64, 3), dtype=np.uint8)
    assert Image.open(gen(controlnet_image=edges, control_mode=1, init_image=photo, strength=0.5)).size == (64, 96)
    neg = {"txt": 0.1 * torch.randn(1, 32, 128, generator=g), "vec": torch.randn(1, 64, generator=g)}
    n1 = gen(controlnet_image=edges, control_mode=1, negative_prompt=neg, true_cfg_scale=3.0, true_cfg_interval=(0, 0.5), output_type="latent")
    assert torch.isfinite(n1).all() and not torch.equal(n1, gen(controlnet_image=edges, control_mode=1, output_type="latent"))
    mask = np.zeros((96, 64), dtype=np.uint8)
    mask[24:72, 16:48] = 255
    mi = gen(controlnet_image=edges, control_mode=1, init_image=photo, inpaint_mask=mask, output_type="latent")
    assert torch.isfinite(mi).all() and not torch.equal(mi, gen(init_image=photo, inpaint_mask=mask, output_type="latent"))
    with pytest.raises(ValueError, match="control_mode"):
        gen(controlnet_image=edges)
