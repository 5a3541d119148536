"""FLUX IP-Adapter on the GPU: the decoupled image attention kernel (csrc/ip_attention.hip) against the fp64 reference and gate of
tests/ip_adapter_ref.py, the engine's adapter launches against the composed oracle of that file (XLabs' processor restated from the oracle's
own blocks: parity with XLabs' code is unpinned), the native CLIP vision tower against transformers, and the pipeline.

Tiny geometry of tests/test_controlnet_gpu.py (hidden 256, 2 heads of 128, 3 double + 4 single blocks) and its gates: rel-L2 <= 1e-2 (bf16
flow), <= 6e-2 against the fp8 oracle and, at calls 0, 7 and 14, distance to the bf16 oracle <= 1.25 x the fp8 oracle's own.  Every parity
case first shows that the oracle with the adapter is >= 10 x its gate away from the oracle without: none of it passes with the term ignored."""
import ctypes as C

import numpy as np
import pytest
import torch

import controlnet_ref as cr
import flux_oracle as fo
import ip_adapter_ref as ir
from test_controlnet_gpu import GATE, NETS, build_main, build_net, calibrate, call_of, inputs, oracles, tiny_config
from test_kontext_gpu import QUANTS, rel_l2, to_dev

pytestmark = pytest.mark.gpu

DEPTH, HID, T = 3, 256, 4


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------------------
def _kernel_buffers(q, k, v, row0, dev, poison=None):
    """the strided device buffers of one case: the image rows sit at rows [row0, row0 + rows) of a longer [B, Ltot, 3 * HD] qkv buffer and
    of a longer x buffer (text rows in front, sentinel rows behind), K / V in buffers of 3 more rows (poison: what those rows hold)"""
    B, rows, HD = q.shape
    nk = k.shape[1]
    g = torch.Generator().manual_seed(rows * 7 + HD + nk)
    Ltot = row0 + rows + 2
    qkv = torch.randn(B, Ltot, 3 * HD, generator=g).bfloat16()
    qkv[:, row0:row0 + rows, :HD] = q
    x = torch.randn(B, Ltot, HD, generator=g).bfloat16()
    kb, vb = (torch.zeros(B, nk + 3, HD, dtype=torch.bfloat16) for _ in range(2))
    if poison is not None:
        kb[:, nk:], vb[:, nk:] = poison, poison
    kb[:, :nk], vb[:, :nk] = k, v
    return qkv.to(dev), x.to(dev), kb.to(dev), vb.to(dev)


@pytest.mark.parametrize("B", [1, 3])
def test_kernel_against_the_gate_and_fused_form(dev, B):
    """every case of the grid: the out-of-place form inside the gate (and rel-L2 <= u: one bf16 rounding of the output is <= u / 2 per element,
    the fp32 arithmetic and the rare one-ulp difference of a qn element are far below that); the fused form == out-of-place + add_scaled bit for
    bit with a scale per sample; scale 0 leaves x as it was; rows outside the image rows are never written"""
    from fluxmi import ops

    worst, worst_l2 = 0.0, 0.0
    for rows, heads, nk, Bc in ir.KERNEL_CASES:
        if Bc != B:
            continue
        row0 = 7 if (rows + heads + nk) % 2 else 0
        q, w, k, v = ir.term_inputs(rows, heads, nk, B, seed=1)
        ref, A, E = ir.term_ref64(q, w, k, v)
        qkv, x, kb, vb = _kernel_buffers(q, k, v, row0, dev)
        HD = heads * 128
        qv = qkv[:, row0:row0 + rows]
        o = ops.ip_attention(qv, w.to(dev), kb, vb, heads, nk)
        what = f"rows {rows} heads {heads} nk {nk} B {B} row0 {row0}"
        n_bad, r = ir.gate_violations(o, ref, A, E)
        l2 = ((o.cpu().double() - ref).norm() / ref.norm()).item()
        worst, worst_l2 = max(worst, r), max(worst_l2, l2)
        assert torch.isfinite(o).all() and n_bad == 0, f"{what}: {n_bad} elements beyond the gate, worst err / bound {r:.3f}"
        assert l2 <= 2.0 ** -8, f"{what}: rel-L2 {l2:.3e}"
        # fused == out-of-place + add_scaled, a scale per sample
        s = torch.tensor([0.7, -1.5, 1.0][:B], dtype=torch.float32, device=dev)
        want = x.clone()
        for b in range(B):
            ops.add_scaled(want[b:b + 1, row0:row0 + rows], o[b:b + 1], s[b:b + 1])
        got = x.clone()
        ops.ip_attention(qv, w.to(dev), kb, vb, heads, nk, x=got[:, row0:row0 + rows], scale=s)
        assert torch.equal(got, want), f"{what}: fused vs out-of-place + add_scaled, rel-L2 {rel_l2(got, want):.3e}"
        assert torch.equal(got[:, :row0], x[:, :row0]) and torch.equal(got[:, row0 + rows:], x[:, row0 + rows:]), f"{what}: wrote outside the image rows"
        assert not torch.equal(got, x)
        zero = x.clone()
        ops.ip_attention(qv, w.to(dev), kb, vb, heads, nk, x=zero[:, row0:row0 + rows], scale=0.0)
        assert torch.equal(zero, x), f"{what}: scale 0 changed x"
    print(f"ip_attention B {B}: worst err / bound {worst:.3f}, worst rel-L2 {worst_l2:.3e} over the grid")


def test_kernel_padding_rows_and_batch_invariance(dev):
    """K / V rows at or beyond Nk hold NaN / 3e38 / zeros: the same bits; a sample alone == the same sample inside B = 3"""
    from fluxmi import ops

    for rows, heads, nk in ((5, 3, 1), (257, 3, 5), (64, 24, 16), (257, 1, 64), (1, 1, 4)):
        B, row0 = 3, 7
        q, w, k, v = ir.term_inputs(rows, heads, nk, B, seed=2)
        outs = []
        for poison in (None, float("nan"), 3e38):
            qkv, x, kb, vb = _kernel_buffers(q, k, v, row0, dev, poison)
            qv = qkv[:, row0:row0 + rows]
            o = ops.ip_attention(qv, w.to(dev), kb, vb, heads, nk)
            ops.ip_attention(qv, w.to(dev), kb, vb, heads, nk, x=x[:, row0:row0 + rows], scale=0.9)
            assert torch.isfinite(o).all() and torch.isfinite(x).all()
            outs.append((o, x))
        for o, x in outs[1:]:
            assert torch.equal(o, outs[0][0]) and torch.equal(x, outs[0][1]), f"rows {rows} heads {heads} nk {nk}: a row beyond Nk reached a result"
        qkv, x, kb, vb = _kernel_buffers(q, k, v, row0, dev)
        for b in range(B):
            alone = ops.ip_attention(qkv[b:b + 1, row0:row0 + rows], w.to(dev), kb[b:b + 1], vb[b:b + 1], heads, nk)
            assert torch.equal(alone[0], outs[0][0][b]), f"rows {rows} heads {heads} nk {nk}: sample {b} alone differs from the batch"


def test_kernel_refusals(dev):
    from fluxmi import ops

    q, w, k, v = ir.term_inputs(5, 1, 4, 1, seed=3)
    qkv, x, kb, vb = _kernel_buffers(q, k, v, 0, dev)
    big = torch.zeros(1, 65, 128, dtype=torch.bfloat16, device=dev)
    for nk, kk in ((0, kb), (65, big)):
        with pytest.raises(RuntimeError, match="Nk"):
            ops.ip_attention(qkv[:, :5], w.to(dev), kk, kk, 1, nk)
    with pytest.raises(ValueError):
        ops.ip_attention(qkv[:, :5], w.to(dev), kb, vb, 1, 9)  # more keys than the buffer holds


# ---- 2. the engine ---------------------------------------------------------------------------------------------------------------------------
def make_kv(B, seed, nk=T, v_gain=4.0, depth=DEPTH):
    g = torch.Generator().manual_seed(4000 + seed)
    return torch.randn(depth, B, nk, HID, generator=g).bfloat16(), (v_gain * torch.randn(depth, B, nk, HID, generator=g)).bfloat16()


def ip_call(k, v, scale, dev):
    from modules.ip_adapter import IPAdapterCall

    return IPAdapterCall(k.to(dev), v.to(dev), scale)


def den(model, d, ts, ip=None, use_graph=True, img=None, **kw):
    return model.denoise(d["img"] if img is None else img, d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts, guidance=3.5, use_graph=use_graph,
                         ip_adapter=ip, **kw)


def ref_den(o, inp, ts, k=None, v=None, sc=None, img=None):
    return ir.denoise(o, inp["img"] if img is None else img, inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], ts, 3.5, k, v, sc)


def timed_steps(model):
    from fluxmi import _lib

    ms, steps = C.c_float(0), C.c_int(0)
    _lib.call("fluxmi_engine_last_timing", model._engine, C.byref(ms), C.byref(steps))
    return steps.value


@pytest.mark.parametrize("qname", ["bf16", "fp8"])
def test_zeroed_v_proj_changes_nothing(dev, qname):
    """an adapter whose v_proj weights and biases are zero (its K / V through the module's own linears): the plain request bit for bit"""
    from fluxmi import synth
    from modules.ip_adapter import IPAdapter

    cfg = tiny_config()
    model, _ = build_main(cfg, QUANTS[qname], dev)
    sd = synth.make_ip_adapter_state_dict(HID, DEPTH, T, seed=1)
    for key in sd:
        if "_v_proj." in key:
            sd[key] = torch.zeros_like(sd[key])
    ad = IPAdapter.from_state_dict(sd).to(device=dev, dtype=torch.bfloat16)
    call = ad.call(image_embeds=torch.randn(2, 768, generator=torch.Generator().manual_seed(3)), scale=[0.7, 1.0, 1.3])
    assert call.k_ip.shape == (DEPTH, 1, 2 * T, HID) and float(call.v_ip.abs().max()) == 0.0 and float(call.k_ip.abs().max()) > 0.0
    B = 2
    d = to_dev(inputs(cfg.params, 64, 64, 32, B, seed=5), dev)
    ts = fo.get_schedule(16, 16)
    lat = calibrate(model, d, ts)
    ts2 = ts[:5]
    plain = den(model, d, ts2, img=lat)
    assert torch.equal(den(model, d, ts2, ip=call, img=lat), plain)
    assert torch.equal(den(model, d, ts2, ip=call, img=lat, use_graph=False), plain)
    t = torch.full((B,), 0.5, dtype=torch.bfloat16, device=dev)
    g = torch.full((B,), 3.5, dtype=torch.bfloat16, device=dev)
    args = (lat, d["img_ids"], d["txt"], d["txt_ids"], t, d["y"], g)
    assert torch.equal(model(*args, ip_adapter=call), model(*args))


@pytest.mark.parametrize("qname", ["bf16", "fp8"])
@pytest.mark.parametrize("shape", [(64, 64, 32, 2, 4), (48, 80, 40, 1, 5)])
def test_forward_matches_oracle_through_calibration(dev, qname, shape):
    H, W, Lt, B, nk = shape
    cfg = tiny_config()
    model, sd = build_main(cfg, QUANTS[qname], dev)
    params = fo.FluxParams(**cfg.params.model_dump())
    o_q = fo.FluxOracle({k: v.clone() for k, v in sd.items()}, params, quantize=QUANTS[qname])
    o_b = fo.FluxOracle({k: v.clone() for k, v in sd.items()}, params, quantize=None)
    inp = inputs(cfg.params, H, W, Lt, B, seed=3)
    d = to_dev(inp, dev)
    k, v = make_kv(B, seed=nk, nk=nk)
    sc = torch.tensor([[0.7, 1.0, 0.4], [1.2, 0.5, 0.9]])[:B]
    call = ip_call(k, v, sc, dev)
    worst = 0.0
    for step in range(15):
        t = torch.full((B,), 1.0 - 0.06 * step, dtype=torch.bfloat16)
        g = torch.full((B,), 3.5, dtype=torch.bfloat16)
        args = (inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], t, inp["y"], g)
        ref = ir.forward(o_q, *args, k, v, sc)
        if step == 0:  # the case shows something: the term moves the oracle by >= 10 x the gate (a throw-away oracle: forward calibrates)
            o_t = fo.FluxOracle({kk: vv.clone() for kk, vv in sd.items()}, params, quantize=QUANTS[qname])
            moved = rel_l2(ref, ir.forward(o_t, *args))
            print(f"[ip-adapter {qname} {shape}] oracle with vs without the adapter: rel-L2 {moved:.3e}")
            assert moved >= 10 * GATE[qname]
        got = model(d["img"], d["img_ids"], d["txt"], d["txt_ids"], t.to(dev), d["y"], g.to(dev), ip_adapter=call)
        assert got.shape == ref.shape and torch.isfinite(got).all()
        e = rel_l2(got, ref)
        worst = max(worst, e)
        print(f"[ip-adapter {qname} {shape}] call {step}: rel-L2 {e:.3e}")
        assert e <= GATE[qname], f"{qname} call {step}: rel-L2 {e:.3e}"
        if QUANTS[qname] is not None and step in (0, 7, 14):
            rb = ir.forward(o_b, *args, k, v, sc)
            d_ref, d_got = rel_l2(ref, rb), rel_l2(got, rb)
            print(f"[ip-adapter {qname} {shape}] call {step}: vs bf16 flow {d_got:.3e}, the fp8 oracle's own {d_ref:.3e}")
            assert d_got <= 1.25 * d_ref, f"{qname} call {step}: vs bf16 flow {d_got:.3e} > 1.25 x {d_ref:.3e}"
    if QUANTS[qname] is not None:
        assert model.calibration_state()[0]
    print(f"[ip-adapter {qname} {shape}] worst rel-L2 over 15 calls: {worst:.3e}")


@pytest.mark.parametrize("qname", ["bf16", "fp8"])
def test_denoise_graph_equals_eager_and_one_graph_serves_scales_and_images(dev, qname):
    cfg = tiny_config()
    model, sd = build_main(cfg, QUANTS[qname], dev)
    params = fo.FluxParams(**cfg.params.model_dump())
    oracle = fo.FluxOracle({k: v.clone() for k, v in sd.items()}, params, quantize=QUANTS[qname])
    B = 1
    inp = inputs(cfg.params, 64, 64, 32, B, seed=7)
    d = to_dev(inp, dev)
    ts = fo.get_schedule(16, 16)
    k, v = make_kv(B, seed=1)
    sc = torch.tensor([[0.8, 0.8, 0.8]])
    ref = ref_den(oracle, inp, ts, k, v, sc)
    plain_ref = ref_den(fo.FluxOracle({kk: vv.clone() for kk, vv in sd.items()}, params, quantize=QUANTS[qname]), inp, ts)
    assert rel_l2(ref, plain_ref) >= 10 * GATE[qname]
    got = den(model, d, ts, ip=ip_call(k, v, 0.8, dev))
    e = rel_l2(got, ref)
    print(f"[ip-adapter {qname}] latents after 16 steps: rel-L2 {e:.3e}")
    assert got.shape == inp["img"].shape and e <= GATE[qname]
    # frozen now.  The first request captures; then two scales (one of them a per-block vector) and another image replay THAT graph -- every
    # step of the request is a timed replay, none an eager warm step -- and each equals its eager run and the oracle at ITS tables
    ts2 = ts[:7]
    den(model, d, ts2, ip=ip_call(k, v, 0.8, dev))
    k2, v2 = make_kv(B, seed=2)
    for kk, vv, s in ((k, v, 0.4), (k, v, [1.0, 0.3, 0.6]), (k2, v2, 0.8)):
        call = ip_call(kk, vv, s, dev)
        a = den(model, d, ts2, ip=call)
        assert timed_steps(model) == 6, "a request with other scales / another image did not replay the captured graph from its first step"
        b = den(model, d, ts2, ip=call, use_graph=False)
        assert torch.equal(a, b), f"scale {s}: graph vs eager rel-L2 {rel_l2(a, b):.3e}"
        from modules.ip_adapter import scale_table

        r = ref_den(oracle, inp, ts2, kk, vv, scale_table(s, DEPTH, B))
        e = rel_l2(a, r)
        print(f"[ip-adapter {qname}] scale {s}: rel-L2 {e:.3e}")
        assert e <= GATE[qname], f"scale {s}: rel-L2 {e:.3e}"
    assert not torch.equal(den(model, d, ts2, ip=ip_call(k, v, 0.4, dev)), den(model, d, ts2, ip=ip_call(k2, v2, 0.4, dev))), "the image does not reach the latents"
    # the python loop over Flux.forward is the same request
    call = ip_call(k, v, 0.4, dev)
    c = d["img"].clone()
    g = torch.full((B,), 3.5, dtype=torch.bfloat16, device=dev)
    for t_curr, t_prev in zip(ts2[:-1], ts2[1:]):
        tv = torch.full((B,), t_curr, dtype=torch.bfloat16, device=dev)
        c = c + (t_prev - t_curr) * model(c, d["img_ids"], d["txt"], d["txt_ids"], tv, d["y"], g, ip_adapter=call)
    assert torch.equal(den(model, d, ts2, ip=call), c)


def test_on_off_on_never_replays_a_stale_graph(dev):
    """adapter on -> off -> on (another Nk in between): every request equals its eager run, and off equals a fresh plain engine"""
    cfg = tiny_config()
    model, _ = build_main(cfg, None, dev)
    fresh, _ = build_main(cfg, None, dev)
    B = 2
    d = to_dev(inputs(cfg.params, 64, 64, 32, B, seed=9), dev)
    ts = fo.get_schedule(4, 16)
    want_plain = den(fresh, d, ts)
    k, v = make_kv(B, seed=1)
    k8, v8 = make_kv(B, seed=2, nk=8)
    want = {}
    for name, call in (("nk4", ip_call(k, v, 0.9, dev)), ("nk8", ip_call(k8, v8, 0.9, dev))):
        want[name] = den(fresh, d, ts, ip=call, use_graph=False)
    assert not torch.equal(want["nk4"], want_plain) and not torch.equal(want["nk4"], want["nk8"])
    assert torch.equal(den(fresh, d, ts), want_plain)
    for name in ("nk4", None, "nk4", "nk8", None, "nk8", "nk4"):
        call = None if name is None else ip_call(k, v, 0.9, dev) if name == "nk4" else ip_call(k8, v8, 0.9, dev)
        got = den(model, d, ts, ip=call)
        exp = want_plain if name is None else want[name]
        assert torch.equal(got, exp), f"{name}: rel-L2 to the expected latents {rel_l2(got, exp):.3e}"
        assert torch.equal(den(model, d, ts, ip=call), got)


def test_guided_branches_carry_their_own_tables(dev, monkeypatch):
    """tests/test_cfg_gpu.py's gate for the bf16 flow: rel-L2 <= max(1e-2, 1.75 x floor), floor = the oracle's own movement when its SDPA is
    replaced by fo.attention_exact"""
    from fluxmi import synth

    cfg = tiny_config()
    B, n, S = 1, 16, 3.5
    ts = fo.get_schedule(n, 16)
    inp = inputs(cfg.params, 64, 64, 32, B, seed=13)
    neg = synth.make_inputs(cfg.params, 64, 64, 32, batch=B, seed=113, real_tokens=4)
    d, dn = to_dev(inp, dev), to_dev(neg, dev)
    model, sd = build_main(cfg, None, dev)
    params = fo.FluxParams(**cfg.params.model_dump())
    mk = lambda: fo.FluxOracle({k: v.clone() for k, v in sd.items()}, params, quantize=None)
    k, v = make_kv(2 * B, seed=5)  # [depth, 2, nk, H]: the prompt branch's tables, then the negative branch's
    sc = torch.tensor([[1.0, 0.6, 0.8], [0.3, 0.9, 0.5]])
    guided = lambda o, kk, vv, ss: ir.denoise_guided(o, inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], neg["txt"], neg["y"], ts, 3.5,
                                                     S, kk, vv, ss)
    ref = guided(mk(), k, v, sc)
    with monkeypatch.context() as mp:
        mp.setattr(fo, "attention", fo.attention_exact)
        floor = rel_l2(guided(mk(), k, v, sc), ref)
    gate = max(1e-2, 1.75 * floor)
    # the case shows something: without the adapter, and with the branches' tables exchanged, the oracle is >= 10 x the gate away
    assert rel_l2(guided(mk(), None, None, None), ref) >= 10 * gate
    assert rel_l2(guided(mk(), k.flip(1), v.flip(1), sc.flip(0)), ref) >= 10 * gate
    kw = dict(neg_txt=dn["txt"], neg_y=dn["y"], cfg_scale=S)
    got = den(model, d, ts, ip=ip_call(k, v, sc, dev), **kw)
    e = rel_l2(got, ref)
    print(f"[ip-adapter cfg bf16] engine vs oracle {e:.3e}; floor {floor:.3e}; gate {gate:.3e}")
    assert got.shape == inp["img"].shape and torch.isfinite(got).all() and e <= gate
    ts2 = ts[:5]
    assert torch.equal(den(model, d, ts2, ip=ip_call(k, v, sc, dev), **kw), den(model, d, ts2, ip=ip_call(k, v, sc, dev), use_graph=False, **kw))


@pytest.mark.parametrize("qname", ["bf16", "fp8"])
def test_with_a_controlnet_in_the_stated_order(dev, qname):
    """block, adapter term, ControlNet residual -- against the composed oracle in that order"""
    cfg = tiny_config()
    model, sd = build_main(cfg, QUANTS[qname], dev)
    net, net_sd = build_net(cfg, NETS["2+2"], QUANTS[qname], dev)
    B = 2
    inp = inputs(cfg.params, 64, 64, 32, B, seed=17)
    d = to_dev(inp, dev)
    k, v = make_kv(B, seed=7, v_gain=16.0)  # (the net's residuals are as large as the stream: a stronger adapter for the same 10 x margin)
    sc = torch.tensor([[0.7, 1.0, 0.4], [1.2, 0.5, 0.9]])
    call, cn = ip_call(k, v, sc, dev), call_of(net, d, 0.7)
    o_main, o_net = oracles(cfg, sd, net_sd, QUANTS[qname])
    for step in range(15):
        t = torch.full((B,), 1.0 - 0.06 * step, dtype=torch.bfloat16)
        g = torch.full((B,), 3.5, dtype=torch.bfloat16)
        args = (inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], t, inp["y"], g)
        Rd, Rs = o_net.residuals(*args, inp["cond"], None)
        if step == 0:
            t_main, t_net = oracles(cfg, sd, net_sd, QUANTS[qname])
            res = t_net.residuals(*args, inp["cond"], None)
            moved = rel_l2(ir.forward(t_main, *args, k, v, sc, cn=(res[0], res[1], 0.7)), ir.forward(oracles(cfg, sd, net_sd, QUANTS[qname])[0], *args, cn=(res[0], res[1], 0.7)))
            assert moved >= 10 * GATE[qname], f"the adapter moves the controlled oracle by {moved:.3e} only"
        ref = ir.forward(o_main, *args, k, v, sc, cn=(Rd, Rs, 0.7))
        got = model(d["img"], d["img_ids"], d["txt"], d["txt_ids"], t.to(dev), d["y"], g.to(dev), ip_adapter=call, controlnet=cn)
        e = rel_l2(got, ref)
        print(f"[ip-adapter + controlnet {qname}] call {step}: rel-L2 {e:.3e}")
        assert e <= GATE[qname], f"{qname} call {step}: rel-L2 {e:.3e}"
    ts2 = fo.get_schedule(16, 16)[:5]
    assert torch.equal(den(model, d, ts2, ip=call, controlnet=cn), den(model, d, ts2, ip=call, controlnet=cn, use_graph=False))


def test_refusals(dev):
    from fluxmi import _lib, ops

    cfg = tiny_config()
    model, _ = build_main(cfg, None, dev)
    net, _ = build_net(cfg, NETS["2+0"], None, dev)
    B = 2
    d = to_dev(inputs(cfg.params, 64, 64, 32, B, seed=21), dev)
    ts = fo.get_schedule(4, 16)
    k, v = make_kv(B, seed=1)
    ok = ip_call(k, v, 1.0, dev)
    # the host wrapper, before any device work
    with pytest.raises(ValueError, match="cache_threshold"):
        den(model, d, ts, ip=ok, cache_threshold=0.1)
    with pytest.raises(ValueError, match="attn_groups"):
        den(model, d, ts, ip=ok, attn_groups=torch.full((1, 48), 1 << 16, dtype=torch.int32, device=dev))
    den(model, d, ts, controlnet=call_of(net, d, 0.5))  # prepares both engines for B = 2
    e, s = model._engine, ops._stream()
    sc = (C.c_float * (B * DEPTH))(*([1.0] * (B * DEPTH)))
    kd, vd = k.to(dev), v.to(dev)
    big = torch.zeros(DEPTH, B, 65, HID, dtype=torch.bfloat16, device=dev)
    set_ip = lambda eng, kk, vv, nk, b: _lib.call("fluxmi_engine_set_ip_adapter", eng, ops._p(kk), ops._p(vv), nk, b, sc, s)
    for nk in (0, 65, -1):
        with pytest.raises(RuntimeError, match="Nk"):
            set_ip(e, big, big, nk, B)
    with pytest.raises(RuntimeError, match="prepared batch"):
        set_ip(e, kd, vd, T, 1)
    with pytest.raises(RuntimeError, match="ControlNet engine"):
        set_ip(net._engine, kd, vd, T, B)
    _lib.call("fluxmi_engine_set_step_cache", e, 0.1, 0)
    with pytest.raises(RuntimeError, match="step caching"):
        set_ip(e, kd, vd, T, B)
    _lib.call("fluxmi_engine_set_step_cache", e, 0.0, 0)
    table = torch.full((B, 32 + 16), 1 << 16, dtype=torch.int32, device=dev)
    _lib.call("fluxmi_engine_set_attn_groups", e, ops._p(table), s)
    with pytest.raises(RuntimeError, match="token-group"):
        set_ip(e, kd, vd, T, B)
    _lib.call("fluxmi_engine_set_attn_groups", e, None, s)
    set_ip(e, kd, vd, T, B)
    with pytest.raises(RuntimeError, match="IP-Adapter is set"):
        _lib.call("fluxmi_engine_run_phase", e, 2, 1, 1, -1, s)
    # state set after the adapter is caught by the call that would run it
    _lib.call("fluxmi_engine_set_step_cache", e, 0.1, 0)
    t = torch.full((B,), 0.5, dtype=torch.bfloat16, device=dev)
    pred = torch.empty(B, 16, 64, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match="step caching"):
        _lib.call("fluxmi_engine_forward", e, ops._p(d["img"]), ops._p(d["txt"]), ops._p(d["y"]), ops._p(t), ops._p(t), ops._p(pred), 2, 0, s)
    _lib.call("fluxmi_engine_set_step_cache", e, 0.0, 0)
    _lib.call("fluxmi_engine_set_ip_adapter", e, None, None, 0, 0, None, s)
    torch.cuda.synchronize()
    assert torch.equal(den(model, d, ts), den(model, d, ts, use_graph=False))


# ---- 3. the CLIP vision tower --------------------------------------------------------------------------------------------------------------------
TINY_CLIP = dict(hidden_size=128, intermediate_size=344, num_hidden_layers=3, num_attention_heads=2, num_channels=3, image_size=224, patch_size=14,
                 hidden_act="quick_gelu", layer_norm_eps=1e-5, projection_dim=96)


def hf_clip(cfg, seed):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection

    from fluxmi import synth

    m = CLIPVisionModelWithProjection(CLIPVisionConfig(**cfg)).eval()
    # transformers' random initialisation shrinks with depth and width (logits near zero); draw O(1) activations instead
    missing, unexpected = m.load_state_dict(synth.make_clip_vision_state_dict(cfg, seed), strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
    return m


def sample_images(n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        a = rng.integers(0, 256, (260 + 37 * i, 300 - 23 * i, 3), dtype=np.uint8)
        a[: a.shape[0] // 2] //= 2
        out.append(a)
    return out


def _clip_gate(cfg, dev, seed, hf_bf16_dev):
    import copy

    from modules.image_embedders import ClipVisionNative
    from modules.ip_adapter import clip_preprocess

    hf = hf_clip(cfg, seed)
    pix = torch.cat([clip_preprocess(im, cfg["image_size"]) for im in sample_images(2, seed)], 0)
    with torch.no_grad():
        r = hf(pixel_values=pix)
        ref, ref_h = r.image_embeds.float(), r.last_hidden_state.float()
        hb = copy.deepcopy(hf).to(device=hf_bf16_dev, dtype=torch.bfloat16)
        y = hb(pixel_values=pix.to(hf_bf16_dev, torch.bfloat16))
        yard, yard_h = y.image_embeds.float().cpu(), y.last_hidden_state.float().cpu()
        del hb
    nat = ClipVisionNative(cfg)
    nat.load_state_dict(hf.state_dict())
    nat = nat.to(device=dev, dtype=torch.bfloat16)
    out = nat(pix.to(dev))
    got, got_h = out["image_embeds"], out["last_hidden_state"]
    assert got.shape == ref.shape and got.dtype == torch.bfloat16 and torch.isfinite(got).all() and got_h.shape == ref_h.shape
    return nat, pix, (rel_l2(got, ref), rel_l2(yard, ref)), (rel_l2(got_h, ref_h), rel_l2(yard_h, ref_h))


def test_clip_tiny_width_vs_transformers(dev):
    nat, pix, (d_nat, d_hf), (h_nat, h_hf) = _clip_gate(TINY_CLIP, dev, 0, torch.device("cpu"))
    print(f"CLIP hidden 128 / 2 heads / 3 layers: image_embeds native {d_nat:.3e} vs transformers bf16 {d_hf:.3e}; last_hidden_state {h_nat:.3e} vs "
          f"{h_hf:.3e} (rel-L2 to fp32)")
    assert d_nat <= 1.5 * d_hf and h_nat <= 1.5 * h_hf
    one = nat(pix[1:].to(dev))["image_embeds"]
    both = nat(pix.to(dev))["image_embeds"]
    assert torch.equal(one[0], both[1])  # batch invariance


def test_clip_full_vit_l14_geometry_vs_transformers(dev):
    """24 x 1024 x 4096, 16 heads of 64, 257 tokens padded to 512, random weights"""
    from modules.image_embedders import CLIP_VIT_L14

    nat, pix, (d_nat, d_hf), (h_nat, h_hf) = _clip_gate(CLIP_VIT_L14, dev, 5, dev)
    assert nat.seq_pad == 512 and nat.num_tokens == 257 and nat.head_pad == 64
    print(f"CLIP ViT-L/14: image_embeds native {d_nat:.3e} vs transformers bf16 {d_hf:.3e}; last_hidden_state {h_nat:.3e} vs {h_hf:.3e} (rel-L2 to fp32)")
    assert d_nat <= 1.5 * d_hf and h_nat <= 1.5 * h_hf


# ---- 4. the pipeline -----------------------------------------------------------------------------------------------------------------------------
def make_pipeline(dev, model, cfg, adapter):
    from flux_pipeline import FluxPipeline

    pipe = FluxPipeline.__new__(FluxPipeline)
    pipe.name, pipe.debug, pipe.dtype, pipe.ae_dtype = "flux-dev", False, torch.bfloat16, torch.bfloat16
    pipe.device_flux = pipe.device_ae = pipe.device_clip = pipe.device_t5 = dev
    pipe.model, pipe.ae, pipe.clip, pipe.t5, pipe.rng = model, None, None, None, torch.Generator(device="cpu")
    pipe.redux, pipe.controlnet, pipe.ip_adapter, pipe.config = None, None, adapter, cfg
    return pipe


def test_pipeline_end_to_end(dev):
    """a tiny CLIP + a tiny adapter through generate(ip_adapter_image=...) == the manual composition (preprocess, tower, projector, K / V,
    Flux.denoise) bit for bit; ip_adapter_image_embeds= equals the image route; two images give Nk = 2 T"""
    from fluxmi import synth
    from modules.image_embedders import ClipVisionNative
    from modules.ip_adapter import IPAdapter, IPAdapterCall, clip_preprocess

    cfg = tiny_config()
    model, _ = build_main(cfg, None, dev)
    ccfg = dict(TINY_CLIP, projection_dim=768)
    clip = ClipVisionNative(ccfg)
    clip.load_state_dict(synth.make_clip_vision_state_dict(ccfg, seed=2))
    ad = IPAdapter.from_state_dict(synth.make_ip_adapter_state_dict(HID, DEPTH, T, seed=3), clip).to(device=dev, dtype=torch.bfloat16)
    pipe = make_pipeline(dev, model, cfg, ad)
    g = torch.Generator().manual_seed(1)
    prompt = {"txt": 0.1 * torch.randn(1, 32, 128, generator=g), "vec": torch.randn(1, 64, generator=g)}
    KW = dict(width=64, height=64, num_steps=4, seed=7, silent=True, output_type="latent")
    im0, im1 = sample_images(2, seed=4)
    plain = pipe.generate(prompt, **KW)
    one = pipe.generate(prompt, ip_adapter_image=im0, ip_adapter_scale=0.8, **KW)
    assert one.shape == plain.shape and torch.isfinite(one).all() and not torch.equal(one, plain)
    # the manual composition
    emb = ad.clip(clip_preprocess(im0).to(dev))["image_embeds"]
    assert emb.shape == (1, 768)
    k, v = ad.kv(emb)
    assert k.shape == (DEPTH, 1, T, HID)
    noise, ts = pipe.preprocess_latent(init_image=None, height=64, width=64, num_steps=4, strength=1.0, generator=pipe.set_seed(7)[0], num_images=1)
    img, img_ids, vec, txt, txt_ids = (t.contiguous() for t in pipe.prepare(noise, prompt))
    lat = model.denoise(img, img_ids, txt, txt_ids, vec, ts, guidance=3.5, ip_adapter=IPAdapterCall(k, v, 0.8))
    assert torch.equal(pipe.unpack(lat.float(), 64, 64), one)
    assert torch.equal(pipe.generate(prompt, ip_adapter_image_embeds=emb, ip_adapter_scale=0.8, **KW), one)
    assert torch.equal(pipe.generate(prompt, ip_adapter_image_embeds=emb.float().cpu(), ip_adapter_scale=[0.8] * DEPTH, **KW), one)
    # two images: their tokens concatenated in list order
    calls = []
    orig = model.denoise
    model.denoise = lambda *a, **kw: (calls.append(kw), orig(*a, **kw))[1]
    try:
        two = pipe.generate(prompt, ip_adapter_image=[im0, im1], ip_adapter_scale=0.8, **KW)
    finally:
        model.denoise = orig
    k2 = calls[0]["ip_adapter"].k_ip
    assert k2.shape == (DEPTH, 1, 2 * T, HID) and torch.equal(k2[:, :, :T], k) and not torch.equal(two, one)
    assert torch.equal(pipe.generate(prompt, **KW), plain)
