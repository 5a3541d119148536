"""Every value of every kernel-selection knob (fluxmi_tuning_t, include/fluxmi.h) at model level, against the contract tests/knob_contract.py
states for it: bit-identical latents, or latents within a stated rel-L2 of the defaults' and within the oracle gate of the flow.

Hidden 256 (2 heads, 2 + 2 blocks), B = 2, 64 x 64 pixels + 32 text tokens (L = 48: even L and Lt, so the fused step keeps its fp8
activations in the row-pair layout).  fp8 flow: calibrated through the denoise loop, then an 8-step frozen denoise per value, hipGraph-
replayed and eager (bit-identical to each other under every value).  bf16 flow (Flux-schnell, nn.Linear everywhere): the same 8-step loop
from the noise -- the flow where split-K, gemm_hybrid and the bf16 tile configs act.  The real-geometry counterpart is in
test_full_geometry_gpu.py (knob_sweep_forward); hidden 4096 (32 heads) is run through calibration and the fused step at the end.
"""
import pytest
import torch

import flux_oracle as fo
import knob_contract as kc
from test_engine_gpu import QUANTS, build, rel_l2, tiny_config, to_dev

pytestmark = pytest.mark.gpu

ORACLE_TOL = {"fp8": 6e-2, "bf16": 1e-2}  # test_engine_gpu.py::test_denoise_loop_matches_oracle


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("flow", ["fp8", "bf16"])
def test_every_knob_value_keeps_its_contract(dev, flow):
    from fluxmi import _lib, synth

    schnell = flow == "bf16"
    cfg = tiny_config(schnell=schnell)
    model, oracle, _ = build(cfg, QUANTS["fp8"] if flow == "fp8" else None, dev)
    B, H, W, Lt = 2, 64, 64, 32
    inp = synth.make_inputs(cfg.params, H, W, Lt, batch=B, seed=11, real_tokens=8)
    d = to_dev(inp, dev)
    n_seq = (H // 16) * (W // 16)
    if flow == "fp8":
        ts = fo.get_schedule(21, n_seq)
        # 13 calibrating calls through the denoise loop on both sides; the 8 frozen steps then start from the ENGINE's latents on both
        lat = model.denoise(d["img"], d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts[:14], guidance=3.5, use_graph=False)
        fo.denoise(oracle, inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], ts[:14], guidance=3.5)
        assert model.calibration_state()[0]
        ts2 = ts[13:]
    else:
        lat = d["img"]
        ts2 = fo.get_schedule(8, n_seq, shift=False)
    assert len(ts2) == 9
    ref_o = fo.denoise(oracle, lat.cpu(), inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], ts2, guidance=3.5)

    def run(use_graph):
        return model.denoise(lat, d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts2, guidance=3.5, use_graph=use_graph)

    base = run(True)
    torch.cuda.synchronize()
    assert _bits_equal(base, run(False)), "defaults: graph replay != eager"
    e_base = rel_l2(base, ref_o)
    assert e_base <= ORACLE_TOL[flow], f"defaults vs oracle: rel-L2 {e_base:.3e}"
    rows, fail = [f"  defaults: latents vs oracle rel-L2 {e_base:.3e} (<= {ORACLE_TOL[flow]:g})"], []
    for knob, value, c in kc.sweep(flow):
        knobs = kc.knobs_of(knob, value, c)
        tag = f"{knob}={value}" + (f" (with {c.knobs_with})" if c.with_ else "")
        try:
            with _lib.tuning(**knobs):
                a = run(True)
                b = run(False)
                torch.cuda.synchronize()
        except RuntimeError as ex:
            rows.append(f"  BAD {tag:44s} refused: {str(ex).splitlines()[0][:160]}")
            fail.append(tag)
            continue
        ok = torch.isfinite(a).all().item() and _bits_equal(a, b)
        same = _bits_equal(a, base)
        e, eo = rel_l2(a, base), rel_l2(a, ref_o)
        if c.kind == "bit":
            ok = ok and same
            what = "BIT held" if same else f"BIT broken: rel-L2 {e:.3e} vs defaults"
        else:
            ok = ok and e <= c.tol and eo <= ORACLE_TOL[flow]
            what = f"rel-L2 {e:.3e} vs defaults (<= {c.tol:g})" + (", bit-identical" if same else "")
        rows.append(f"  {'ok ' if ok else 'BAD'} {tag:44s} {what}; vs oracle {eo:.3e}; graph == eager {_bits_equal(a, b)}")
        if not ok:
            fail.append(tag)
    # the struct is back at its defaults: the re-captured graph computes the defaults' bits again
    assert _bits_equal(run(True), base)
    print(f"\n[{flow} flow, hidden 256, B = {B}, L = {Lt + n_seq}, 8 frozen steps per value]\n" + "\n".join(rows))
    assert not fail, f"{len(fail)} knob value(s) broke their contract: {fail}"


def test_hidden_4096_through_calibration_and_the_fused_step(dev):
    """A model wider than Flux-dev: hidden 4096 = 32 heads x 128, mlp 16384, 1 + 1 blocks, L = 304 (even: the fused step would take the
    row-pair activations, which the LayerNorm kernel that serves this width cannot write -- the engine keeps plain rows there).  15 calls
    through calibration against the CPU oracle, then fused (mode 1) against unfused-frozen (mode 2), at the gates of
    test_forward_matches_oracle_through_calibration / test_full_width_blocks_match_oracle."""
    import util
    from fluxmi import synth

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    p = cfg.params
    p.hidden_size, p.num_heads, p.depth, p.depth_single_blocks = 4096, 32, 1, 1
    model, oracle, sd = build(cfg, QUANTS["fp8"], dev, seed=2)
    oracle_bf16 = fo.FluxOracle({k: v.clone() for k, v in sd.items()}, fo.FluxParams(**p.model_dump()), quantize=None)
    del sd
    H, W, Lt, B = 256, 256, 48, 1  # Li = 256, L = 304
    inp = synth.make_inputs(p, H, W, Lt, batch=B, seed=6, real_tokens=16)
    d = to_dev(inp, dev)
    g = torch.full((B,), 3.5, dtype=torch.bfloat16)
    worst = 0.0
    for step in range(15):
        t = torch.full((B,), 1.0 - 0.05 * step, dtype=torch.bfloat16)
        ref = oracle.forward(inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], t, inp["y"], g)
        got = model(d["img"], d["img_ids"], d["txt"], d["txt_ids"], t.to(dev), d["y"], g.to(dev))
        assert torch.isfinite(got).all()
        e = rel_l2(got, ref)
        worst = max(worst, e)
        assert e <= 6e-2, f"hidden 4096 call {step}: rel-L2 vs fp8 oracle {e:.3e}"
        if step in (0, 14):
            rb = oracle_bf16.forward(inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], t, inp["y"], g)
            d_ref, d_got = rel_l2(ref, rb), rel_l2(got, rb)
            assert d_got <= 1.25 * d_ref, f"hidden 4096 call {step}: vs bf16 flow {d_got:.3e} > 1.25 x {d_ref:.3e}"
    assert model.calibration_state()[0]
    t = torch.full((B,), 0.3, dtype=torch.bfloat16, device=dev)
    args = (d["img"], d["img_ids"], d["txt"], d["txt_ids"], t, d["y"], g.to(dev))
    a, b = model(*args, mode=1), model(*args, mode=2)
    assert torch.isfinite(a).all()
    e12 = rel_l2(a, b)
    print(f"[hidden 4096] worst rel-L2 over 15 calls vs oracle: {worst:.3e}; fused vs unfused rel-L2 {e12:.3e}")
    assert e12 <= 2e-3
