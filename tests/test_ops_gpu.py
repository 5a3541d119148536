"""GPU parity tests: every HIP kernel (through the C ABI) against the CPU oracle on seeded inputs.

Tolerances (stated per test):
  * fp8 / bf16 casts, quantise, amax, scale state machine: bit-exact
  * GEMM on identical quantised operands: <= 1 bf16 ulp of the fp64 result, >= 99 % bit-exact
  * fused elementwise chains: <= 1 bf16 ulp (reduction order / exp approximation), >= 99.9 % bit-exact
  * flow attention: EVERY element within 1.25 * max(1, r_model) * u (|ref| + A) of an fp64 softmax, u = 2^-8, A = softmax |V|, and rel-L2
    within 1.25 x that of a CPU model with the kernel's documented rounding points (fp32 scores, bf16 P, one bf16 output rounding; r_model =
    the model's own worst err / bound): tests/attention_ref.py, whose gate tests/test_attention_ref_cpu.py shows to reject a 2 % scale error,
    a dropped or admitted key, a wrong k-slot and exchanged heads at every length; fused fp8 output == quantise(own bf16 output) bit for bit
"""
import math

import pytest
import torch
import torch.nn.functional as F

import attention_ref as ar
import flux_oracle as fo
from parity_util import accum_noise, assert_bf16_close, assert_close_mag, assert_f8_close, f8_ulp_diff, round_fp64_to_bf16, ulp_diff

pytestmark = pytest.mark.gpu

E4M3, E5M2 = 0, 1
F8T = {E4M3: torch.float8_e4m3fn, E5M2: torch.float8_e5m2}
F8MAX = {E4M3: 448.0, E5M2: 57344.0}


@pytest.fixture(scope="module")
def ops(dev):
    from fluxmi import ops as _ops

    return _ops


def all_bf16():
    x = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    return x[~torch.isnan(x)]


def scalar(v, dev):
    return torch.tensor(float(v), dtype=torch.float32, device=dev)


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [E5M2, E4M3])
@pytest.mark.parametrize("scale", [1.0, 3.3, 448.0, 57344.0, 0.0123])
def test_quantize_exhaustive(ops, dev, fmt, scale):
    """G1: every bf16 input through q = fp8(clamp(bf16(x*scale))) -- bit-exact vs float8_quantize.py:217-218."""
    x = all_bf16()
    x = x[: (x.numel() // 8) * 8].reshape(-1, 8)
    s = torch.tensor(scale, dtype=torch.float32)
    ref = fo.to_fp8_saturated(x, s, F8MAX[fmt]).to(F8T[fmt])
    got = ops.quantize_act(x.to(dev), s.to(dev), fmt).cpu()
    bad = (got.view(torch.uint8) != ref.view(torch.uint8))
    assert not bad.any(), f"{bad.sum().item()} mismatching bytes, first inputs {x[bad][:5].float().tolist()}"


def test_amax_and_calibration_trace(ops, dev):
    """G2/G3: amax + the 12-trial running-max scale state machine (float8_quantize.py:214-246), bit-exact."""
    torch.manual_seed(1)
    st = fo.F8LinearState(torch.randn(16, 64).bfloat16(), None)
    trials = torch.zeros(12, dtype=torch.float32, device=dev)
    scale = torch.zeros((), dtype=torch.float32, device=dev)
    recip = torch.zeros((), dtype=torch.float32, device=dev)
    for call in range(15):
        x = (torch.randn(40, 64) * (0.5 + 3.0 * ((call * 7) % 5))).bfloat16()
        if call == 3:
            x = x * 1e-3  # amax < 1 -> scale clamps at max_val
        ref_q = st.quantize_input(x)
        if call <= 12:
            a = ops.amax(x.to(dev))
            assert a.item() == x.abs().max().float().item()
            ops.calib_update(a, trials, scale, recip, call, 12, 57344.0)
        assert scale.item() == st.input_scale.item(), f"call {call}: scale {scale.item()} vs {st.input_scale.item()}"
        assert recip.item() == st.input_scale_reciprocal.item()
        got_q = ops.quantize_act(x.to(dev), scale, E5M2).cpu()
        assert torch.equal(got_q.view(torch.uint8), ref_q.view(torch.uint8)), f"call {call}"
    assert st.input_scale_initialized and torch.equal(trials.cpu(), st.input_amax_trials)


@pytest.mark.parametrize("amax", [0.0, 1e-13, 0.5, 1.0, 2.0, 448.0, 1e5])
def test_amax_to_scale_edges(ops, dev, amax):
    for max_val in (448.0, 57344.0):
        trials = torch.zeros(12, dtype=torch.float32, device=dev)
        scale, recip = scalar(0, dev), scalar(0, dev)
        ops.calib_update(scalar(amax, dev), trials, scale, recip, 0, 12, max_val)
        ref = fo.amax_to_scale(torch.tensor(amax, dtype=torch.float32), max_val)
        assert scale.item() == ref.item() and recip.item() == ref.reciprocal().item()


def test_quantize_weight(ops, dev):
    torch.manual_seed(2)
    for amp in (0.02, 1.0, 30.0):
        w = (torch.randn(192, 256) * amp).bfloat16()
        w[5, 7] = w.abs().max() * 4
        q_ref, s_ref, r_ref = fo.quantize_weight(w)
        q, s, r = ops.quantize_weight(w.to(dev))
        assert s.item() == s_ref.item() and r.item() == r_ref.item()
        assert torch.equal(q.cpu().view(torch.uint8), q_ref.view(torch.uint8))


# ------------------------------------------------------------------------------------------------
def make_f8_problem(M, N, K, fmt, seed):
    g = torch.Generator().manual_seed(seed)
    a = (torch.randn(M, K, generator=g) * 2.0).bfloat16()
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16()
    a[:, 3] += 1.5  # asymmetric data: catches row/col or k permutation mistakes
    w[1] *= 3.0
    sa = fo.amax_to_scale(a.abs().max().float(), F8MAX[fmt])
    a8 = fo.to_fp8_saturated(a, sa, F8MAX[fmt]).to(F8T[fmt])
    w8, sb, sbr = fo.quantize_weight(w)
    bias = torch.randn(N, generator=g).bfloat16()
    return a8, w8, sa.reciprocal(), sbr, bias


def _f8_gemm_cases():
    """(tile config, shape, activation format): every shape a kernel can tile (config 2 / 15 step K by 128 bytes, 16 by 256), e4m3
    activations on one representative shape per kernel"""
    shapes = [(256, 256, 64), (256, 256, 128), (512, 768, 256), (300, 512, 384), (37, 256, 3072), (1024, 1024, 1024)]
    out = []
    for cfg in (2, 13, 15, 16, 100):
        for shape in shapes:
            K = shape[2]
            if (K % 128 and cfg in (2, 15)) or (K % 256 and cfg == 16):
                continue
            out.append((cfg, shape, E5M2))
            if shape == (512, 768, 256) and cfg != 15:
                out.append((cfg, shape, E4M3))
    return out


@pytest.mark.parametrize("cfg,shape,fmt", _f8_gemm_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_f8_gemm(ops, dev, cfg, shape, fmt):
    """K1: fp8 GEMM on identical quantised operands vs fp64 (float8_quantize.py:284-292): <= 1 bf16 ulp."""
    M, N, K = shape
    a8, w8, sar, sbr, bias = make_f8_problem(M, N, K, fmt, seed=M + N + K)
    ref = round_fp64_to_bf16(fo.scaled_mm_fp64(a8, w8, sar, sbr, bias))
    out = ops.linear(a8.to(dev), w8.to(dev), bias.to(dev), sar.to(dev), sbr.to(dev), tile_cfg=cfg)
    torch.cuda.synchronize()
    noise = accum_noise(a8, w8, sar * sbr)
    assert_close_mag(out, ref, mag=noise, ulps=1.05, min_exact=0.98, what=f"f8 gemm cfg={cfg} {shape} vs fp64")
    # and against torch's own CPU _scaled_mm (what the reference executes; fp32 accumulation like ours)
    ref2 = fo.scaled_mm_ref(a8, w8, sar, sbr, bias)
    assert_close_mag(out, ref2, mag=noise, ulps=1.05, min_exact=0.98, what="vs torch._scaled_mm")


PROD_SHAPES = {  # (groups of M rows, N, K): the launches of one Flux-dev 1024x1024 step
    "double.qkv": ((512, 4096), 9216, 3072), "double.proj": ((512, 4096), 3072, 3072), "double.mlp0": ((512, 4096), 12288, 3072),
    "double.mlp2": ((512, 4096), 3072, 12288), "single.linear1": ((4608,), 21504, 3072), "single.linear2": ((4608,), 3072, 15360),
    "768.qkv": ((512, 2304), 9216, 3072), "768.linear2": ((2816,), 3072, 15360),
}


@pytest.mark.parametrize("which", list(PROD_SHAPES))
def test_f8_gemm_production_shapes_auto_dispatch(ops, dev, which):
    """The shapes and the DISPATCH the engine really uses (tile_cfg = -1: cost model, grouped txt + img launch, 256x256 ping-pong for
    K = 3072, one-wave-per-SIMD for K >= 8192, the hybrid 256x256 + 128x128 peel of a thin last round) on identical fp8 operands:
    <= 1 bf16 ulp of an fp64 evaluation on sampled rows (tile borders included), every column.   float8_quantize.py:284-292"""
    from fluxmi import _lib

    Ms, N, K = PROD_SHAPES[which]
    g = torch.Generator().manual_seed(N + K + sum(Ms))
    groups, keep, checks = [], [], []
    for gi, M in enumerate(Ms):
        a = (torch.randn(M, K, generator=g) * 2.0).bfloat16()
        a[:, 3] += 1.5
        w = (torch.randn(N, K, generator=g) * 0.05).bfloat16()
        w[1] *= 3.0
        sa = fo.amax_to_scale(a.abs().max().float(), 57344.0)
        a8 = fo.to_fp8_saturated(a, sa, 57344.0).to(torch.float8_e5m2)
        w8, sb, sbr = fo.quantize_weight(w)
        bias = torch.randn(N, generator=g).bfloat16()
        sar = sa.reciprocal()
        dv = [t.to(dev) for t in (a8, w8, bias, sar, sbr)]
        out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        keep += dv + [out]
        groups.append(ops.make_group(ops._p(dv[0]), ops._p(dv[1]), ops._p(dv[2]), ops._p(dv[3]), ops._p(dv[4]), ops._p(out), M, K, N))
        rows = sorted(set([0, 1, 127, 128, 255, 256, M // 2, M - 257, M - 256, M - 129, M - 128, M - 2, M - 1] + list(range(7, M, max(1, M // 23)))))
        rows = torch.tensor([r for r in rows if 0 <= r < M])
        checks.append((out, a8, w8, sar, sbr, bias, rows))
    ops.gemm_grouped(groups, N, K, True, E5M2, _lib.EPI_BF16, -1)
    torch.cuda.synchronize()
    for gi, (out, a8, w8, sar, sbr, bias, rows) in enumerate(checks):
        a = a8[rows]
        ref = round_fp64_to_bf16(fo.scaled_mm_fp64(a, w8, sar, sbr, bias))
        noise = accum_noise(a, w8, sar * sbr)
        ex = assert_close_mag(out.cpu()[rows], ref, mag=noise, ulps=1.05, min_exact=0.98, what=f"{which} group {gi} M={out.shape[0]} N={N} K={K} vs fp64")
        print(f"{which} group {gi}: {len(rows)} rows x {N} columns within 1 bf16 ulp of fp64, bit-exact {ex:.5f}")


@pytest.mark.parametrize("case", ["bf16 linear2 M=512", "bf16 mlp2 txt+img", "bf16 mlp2 ragged M", "fp8 forced S=5"])
def test_gemm_split_k(ops, dev, case):
    """Small-M launches: `S` workgroups per 256x256 tile, each over its own K range, fp32 partial tiles + a reduce pass that applies the
    epilogue (gemm_pp.hip).  The shapes the auto dispatch splits (bf16, <= 128 tiles: Flux-schnell 256x256 = BASELINE configs[0], the
    text encoders) with both epilogues, grouped txt + img launches, a ragged M, and a forced split of an fp8 problem (the per-tensor scales
    are then applied by the reduce pass): every row within 1 bf16 ulp of fp64; 5 launches bit-identical; the auto dispatch == the forced
    split it is expected to choose."""
    from fluxmi import _lib

    g = torch.Generator().manual_seed(len(case))
    cases = {"bf16 linear2 M=512": ((512,), 3072, 15360, False, _lib.EPI_GATE_RESID, 10), "bf16 mlp2 txt+img": ((256, 256), 3072, 12288, False, _lib.EPI_GATE_RESID, 8),
             "bf16 mlp2 ragged M": ((300, 77), 3072, 12288, False, _lib.EPI_BF16, 7), "fp8 forced S=5": ((512,), 1024, 4096, True, _lib.EPI_BF16, 5)}
    Ms, N, K, fp8, epi, S = cases[case]
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16()
    bias, gate = torch.randn(N, generator=g).bfloat16(), torch.randn(N, generator=g).bfloat16()
    if fp8:
        w8, sb, sbr = fo.quantize_weight(w)
        dw, dsbr = w8.to(dev), sbr.to(dev)
    else:
        dw, dsbr = w.to(dev), None
    dbias, dgate = bias.to(dev), gate.to(dev)
    groups, keep, checks = [], [], []
    for M in Ms:
        a = torch.randn(M, K, generator=g).bfloat16()
        a[:, 3] += 1.5
        x = torch.randn(M, N, generator=g).bfloat16()
        if fp8:
            sa = fo.amax_to_scale(a.abs().max().float(), 57344.0)
            a_op = fo.to_fp8_saturated(a, sa, 57344.0).to(torch.float8_e5m2)
            sar = sa.reciprocal()
            dsar = sar.to(dev)
        else:
            a_op, sar, dsar = a, None, None
        da, dx = a_op.to(dev), x.to(dev)
        out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        keep += [da, dx, out, dsar]
        kw = dict(gate=ops._p(dgate), resid=ops._p(dx), ldr=N) if epi == _lib.EPI_GATE_RESID else {}
        groups.append(ops.make_group(ops._p(da), ops._p(dw), ops._p(dbias), ops._p(dsar) if fp8 else None, ops._p(dsbr) if fp8 else None, ops._p(out), M, K, N, **kw))
        checks.append((out, a_op, sar, x))
    runs = []
    for cfg in [113 + S] * 5 + ([-1] if not fp8 else []):
        for c in checks:
            c[0].fill_(float("nan"))
        ops.gemm_grouped(groups, N, K, fp8, E5M2, epi, cfg)
        torch.cuda.synchronize()
        runs.append([c[0].clone() for c in checks])
    for r in runs[1:]:
        for a_, b_ in zip(runs[0], r):
            assert torch.equal(a_.view(torch.int16), b_.view(torch.int16)), f"{case}: split-K launches differ (the last one is the auto dispatch)"
    for gi, (out, a_op, sar, x) in enumerate(checks):
        wref = w8 if fp8 else w
        acc = a_op.double() @ wref.double().T
        sc = float(sar * sbr) if fp8 else 1.0
        h = round_fp64_to_bf16(acc * sc + bias.double())
        noise = accum_noise(a_op, wref, sc)
        if epi == _lib.EPI_GATE_RESID:
            ref = (x.float() + (gate.float() * h.float()).bfloat16().float()).bfloat16()
            gh = (gate.float() * h.float()).abs().double()
            mag = torch.maximum(torch.maximum(noise * gate.float().abs()[None, :].double(), gh), x.double().abs())
            ex = assert_close_mag(runs[0][gi], ref, mag=mag, ulps=2.05, min_exact=0.95, what=f"split-K {case} group {gi}")
        else:
            ex = assert_close_mag(runs[0][gi], h, mag=noise, ulps=1.05, min_exact=0.98, what=f"split-K {case} group {gi}")
        print(f"split-K {case} group {gi} (M={out.shape[0]}): bit-exact vs fp64 {ex:.5f}")


@pytest.mark.parametrize("cfg", [2, 13, 15, 100])
def test_bf16_gemm(ops, dev, cfg):
    torch.manual_seed(5)
    M, N, K = 320, 512, 192
    a = torch.randn(M, K).bfloat16()
    w = (torch.randn(N, K) * 0.1).bfloat16()
    a[:, 1] += 2
    bias = torch.randn(N).bfloat16()
    ref = round_fp64_to_bf16(a.double() @ w.double().T + bias.double())
    out = ops.linear(a.to(dev), w.to(dev), bias.to(dev), tile_cfg=cfg)
    assert_close_mag(out, ref, mag=accum_noise(a, w, 1.0), ulps=1, min_exact=0.99, what=f"bf16 gemm cfg={cfg}")


@pytest.mark.parametrize("case", ["bf16", "bf16 ragged + V^T", "gate_resid txt+img", "gelu table", "split + V^T", "split 2 groups ragged"])
def test_gemm_persistent_matches_ping_pong(ops, dev, case):
    """Tile config 18 (gemm_persist.hip: one workgroup per CU walks a static tile list, the LDS ring never drains, epilogue through a
    4 KiB per-wave scratch) runs the K loop of config 13 in the same order with the same rounding points, so every output byte must be
    IDENTICAL to config 13's -- plain bf16 rows, the fused V^T layout, gate*y+x in place, the table-driven GELU -> fp8 epilogue, the
    qkv|mlp split of SingleStreamBlock.linear1 -- for ragged M (rows past M read as zero through the buffer descriptor, stores
    masked), several groups with their own weights, and tile counts from fewer than the 256 CUs (one tile per workgroup) to five tiles
    per workgroup (table and non-table tiles alternating inside one workgroup's list).          float8_quantize.py:284-292,
    flux_model.py:301,387-396,471-484"""
    from fluxmi import _lib

    torch.manual_seed(23)
    Hh = 512                       # "hidden": q | k | v blocks of 512 columns = 4 heads of 128
    K = 768
    one, qs = torch.tensor(1.0, device=dev), torch.tensor(41.0, device=dev)
    lut = ops.build_quant_lut(qs, E5M2, act=1)
    spec = {
        "bf16": (_lib.EPI_BF16, [1300], 2048, False),
        "bf16 ragged + V^T": (_lib.EPI_BF16, [777, 130], 3 * Hh, True),
        "gate_resid txt+img": (_lib.EPI_GATE_RESID, [512, 4096], 3072, False),
        "gelu table": (_lib.EPI_GELU_QUANT, [2100], 8192, False),               # 288 tiles: two per workgroup for some
        "split + V^T": (_lib.EPI_SPLIT, [4608], 3 * Hh + 16896, True),            # 1296 tiles: five per workgroup, table and plain tiles mixed
        "split 2 groups ragged": (_lib.EPI_SPLIT, [1000, 333], 3 * Hh + 2048, False),
    }
    epi, Ms, N, vt = spec[case]
    results = {}
    for cfg in (13, 18):
        torch.manual_seed(23)
        groups, keep, outs = [], [], []
        for gi, M in enumerate(Ms):
            a = (torch.randn(M, K, device=dev) * 2).to(torch.float8_e5m2)
            w = (torch.randn(N, K, device=dev) * 0.5).to(torch.float8_e4m3fn)
            bias = torch.randn(N, device=dev).bfloat16() if gi == 0 else None   # the second group has no bias
            sar = torch.tensor(0.37 + gi, device=dev)
            kw = {}
            if epi == _lib.EPI_BF16:
                o = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
            elif epi == _lib.EPI_GELU_QUANT:
                o = torch.zeros(M, N, dtype=torch.uint8, device=dev).view(torch.float8_e5m2)
                kw = dict(q_scale=qs.data_ptr(), q_lut=lut.data_ptr())
            elif epi == _lib.EPI_GATE_RESID:
                o = torch.randn(M, N, device=dev).bfloat16()
                gate = torch.randn(N, device=dev).bfloat16()
                keep.append(gate)
                kw = dict(gate=gate.data_ptr(), resid=o.data_ptr(), ldr=N)
            else:
                o = torch.full((M, 3 * Hh), float("nan"), dtype=torch.bfloat16, device=dev)
                o2 = torch.zeros(M, Hh + (N - 3 * Hh), dtype=torch.uint8, device=dev).view(torch.float8_e5m2)
                outs.append(o2)
                kw = dict(C2=o2.data_ptr(), ldc2=o2.stride(0), split_n=3 * Hh, c2_col0=Hh, q_scale=qs.data_ptr(), q_lut=lut.data_ptr())
            if vt:
                Lp = (M + 63) // 64 * 64
                vt_t = torch.full((Hh, Lp), float("nan"), dtype=torch.bfloat16, device=dev)
                outs.append(vt_t)
                kw.update(vt_out=vt_t.data_ptr(), vt_ld=Lp, tok0=0, vt_rows=Lp, kv_col0=Hh, heads=Hh // 128)
            keep += [a, w, bias, sar]
            outs.append(o)
            groups.append(ops.make_group(a.data_ptr(), w.data_ptr(), bias.data_ptr() if bias is not None else None, sar.data_ptr(), one.data_ptr(),
                                         o.data_ptr(), M, K, o.stride(0), **kw))
        ops.gemm_grouped(groups, N, K, True, E5M2, epi, cfg)
        if cfg == 18:  # a second launch on the same buffers (gate*y+x: on a fresh residual) must reproduce itself
            torch.cuda.synchronize()
        results[cfg] = [o.clone().view(torch.uint8) for o in outs]
    for i, (x13, x18) in enumerate(zip(results[13], results[18])):
        same = (x13 == x18).float().mean().item()
        assert same == 1.0, f"{case}: output {i} of the persistent kernel differs from config 13 on {1 - same:.2e} of the bytes"
    if vt:  # the V columns live in vt_out only: both kernels leave those columns of C untouched (NaN fill), everything else is finite
        assert torch.isfinite(results[18][-1].view(torch.bfloat16).float()[:, :Hh]).all()


@pytest.mark.parametrize("epi_name", ["bf16", "gate_resid", "gelu table", "split"])
def test_gemm_persistent_store_canary(ops, dev, epi_name):
    """Canary for the code-generation hazards gemm_persist.hip works around: hipcc 7.2 omits the data-VGPR-overwrite hazard of
    a 128-bit buffer_store whose soffset is a register -- 300 to 35 000 wrong bytes PER LAUNCH, different ones every time -- so the kernel
    keeps soffset at 0 and nothing at build time would notice a toolchain that brings the problem back.  Twenty back-to-back launches of the
    persistent kernel (tile config 18) per epilogue, on row counts whose tile bands are PARTIAL (7 + 11 row tiles: 18 % PS_GROUP_M(4) != 0,
    ragged last tiles), every output byte of every launch against config 13's; and the one-wave-per-SIMD kernel (config 16) on a launch whose
    last band is partial for ITS band height (7 row tiles % W1_GROUP_M(6) = 1).                             float8_quantize.py:284-292"""
    from fluxmi import _lib

    torch.manual_seed(29)
    Hh, K = 512, 1024
    one, qs = torch.tensor(1.0, device=dev), torch.tensor(41.0, device=dev)
    lut = ops.build_quant_lut(qs, E5M2, act=1)
    epi, N = {"bf16": (_lib.EPI_BF16, 2048), "gate_resid": (_lib.EPI_GATE_RESID, 3072), "gelu table": (_lib.EPI_GELU_QUANT, 4096),
              "split": (_lib.EPI_SPLIT, 3 * Hh + 4096)}[epi_name]
    Ms = [1800, 2600]  # 8 + 11 row tiles, both ragged
    a = [(torch.randn(M, K, device=dev) * 2).to(torch.float8_e5m2) for M in Ms]
    w = [(torch.randn(N, K, device=dev) * 0.5).to(torch.float8_e4m3fn) for _ in Ms]
    bias = torch.randn(N, device=dev).bfloat16()
    gate = torch.randn(N, device=dev).bfloat16()
    resid = [torch.randn(M, N, device=dev).bfloat16() for M in Ms]
    sar = torch.tensor(0.41, device=dev)

    def launch(cfg):
        groups, outs = [], []
        for gi, M in enumerate(Ms):
            kw = {}
            if epi == _lib.EPI_BF16:
                o = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
            elif epi == _lib.EPI_GELU_QUANT:
                o = torch.zeros(M, N, dtype=torch.uint8, device=dev).view(torch.float8_e5m2)
                kw = dict(q_scale=qs.data_ptr(), q_lut=lut.data_ptr())
            elif epi == _lib.EPI_GATE_RESID:
                o = resid[gi].clone()
                kw = dict(gate=gate.data_ptr(), resid=o.data_ptr(), ldr=N)
            else:
                o = torch.full((M, 3 * Hh), float("nan"), dtype=torch.bfloat16, device=dev)
                o2 = torch.zeros(M, Hh + (N - 3 * Hh), dtype=torch.uint8, device=dev).view(torch.float8_e5m2)
                outs.append(o2)
                kw = dict(C2=o2.data_ptr(), ldc2=o2.stride(0), split_n=3 * Hh, c2_col0=Hh, q_scale=qs.data_ptr(), q_lut=lut.data_ptr())
            outs.append(o)
            groups.append(ops.make_group(a[gi].data_ptr(), w[gi].data_ptr(), bias.data_ptr(), sar.data_ptr(), one.data_ptr(), o.data_ptr(), M, K, o.stride(0), **kw))
        ops.gemm_grouped(groups, N, K, True, E5M2, epi, cfg)
        torch.cuda.synchronize()
        return [o.view(torch.uint8).clone() for o in outs]

    ref = launch(13)
    bad = 0
    for it in range(20):
        for x13, x18 in zip(ref, launch(18)):
            bad += int((x13 != x18).sum())
    assert bad == 0, f"{epi_name}: {bad} bytes of 20 persistent-kernel launches differ from config 13"
    if epi in (_lib.EPI_BF16, _lib.EPI_GATE_RESID):  # config 16 carries these two epilogues in the step (mlp.2, linear2): partial last band of 6
        Ms[:] = [1700]  # 7 row tiles
        a[:] = [(torch.randn(1700, K, device=dev) * 2).to(torch.float8_e5m2)]
        resid[:] = [torch.randn(1700, N, device=dev).bfloat16()]
        ref = launch(13)
        for it in range(5):
            for x13, x16 in zip(ref, launch(16)):
                assert torch.equal(x13, x16), f"{epi_name}: config 16 differs from config 13 on a launch with a partial last tile band"


@pytest.mark.parametrize("Ms", [[512, 2304], [2816], [1000, 77]])
def test_gemm_tile_config_17_matches_16(ops, dev, Ms):
    """Tile config 17 (round 5) = the one-wave-per-SIMD kernel on 192 x 256 tiles for gate*y+x launches whose 256-row tiling fills less than one
    round of the CUs (Flux-dev 768^2: mlp.2 grouped txt + img, linear2).  Same K loop, same MFMAs in the same order: every output byte must
    equal config 16's and config 13's -- ragged last tiles (2816 = 14 x 192 + 128; 77 rows), two groups with their own weights, and the
    automatic dispatch (tile_cfg -1 with and without fluxmi_tuning_t.gemm_tile192), which takes it for these shapes at K >= 8192.
    float8_quantize.py:284-292, flux_model.py:387-396,484"""
    from fluxmi import _lib

    torch.manual_seed(31)
    N, K = 3072, 8192
    one = torch.tensor(1.0, device=dev)
    a = [(torch.randn(M, K, device=dev) * 2).to(torch.float8_e5m2) for M in Ms]
    w = [(torch.randn(N, K, device=dev) * 0.5).to(torch.float8_e4m3fn) for _ in Ms]
    bias = torch.randn(N, device=dev).bfloat16()
    gate = torch.randn(N, device=dev).bfloat16()
    resid = [torch.randn(M, N, device=dev).bfloat16() for M in Ms]
    sar = torch.tensor(0.013, device=dev)

    def launch(cfg):
        outs, groups = [], []
        for gi, M in enumerate(Ms):
            o = resid[gi].clone()
            outs.append(o)
            groups.append(ops.make_group(a[gi].data_ptr(), w[gi].data_ptr(), bias.data_ptr() if gi == 0 else None, sar.data_ptr(), one.data_ptr(), o.data_ptr(), M, K,
                                         N, gate=gate.data_ptr(), resid=o.data_ptr(), ldr=N))
        ops.gemm_grouped(groups, N, K, True, E5M2, _lib.EPI_GATE_RESID, cfg)
        torch.cuda.synchronize()
        return [o.view(torch.int16).clone() for o in outs]

    ref = launch(16)
    for cfg in (17, 13, -1):
        for x, y in zip(ref, launch(cfg)):
            assert torch.equal(x, y), f"tile config {cfg} differs from config 16 (Ms = {Ms})"
    with _lib.tuning(gemm_tile192=0):
        for x, y in zip(ref, launch(-1)):
            assert torch.equal(x, y)
    for x in ref:
        assert torch.isfinite(x.view(torch.bfloat16).float()).all()


@pytest.mark.parametrize("M,N,K", [(2048, 3072, 4096), (4096, 3072, 3072), (16384, 3072, 64), (1000, 3072, 15360), (4096, 64, 3072)])
def test_bf16_tile_configs_are_bit_identical(ops, dev, M, N, K):
    """Round 6: every bf16 tile config sums K in ONE order -- the 128-byte-K-step tiles (configs 2 / 15) issue their MFMAs over the same 16-byte
    chunk pairs as the 64-byte-K-step 256 x 256 kernels (13 / 16 / 17), so a bf16 linear's bits do not depend on which tile the dispatcher
    picks for the row count (round 5: ~3e-4 of the outputs differed in the last bit and, through img_in, a sample's latents followed its batch;
    profiles/r05_batch_invariance.txt).  Plain and gate*y+x epilogues, a ragged M, and the automatic choice on a quarter of the rows.
    reference: F.linear on bf16 (flux_model.py:154-155, 356-400), no cross-row operation."""
    from fluxmi import _lib

    torch.manual_seed(5)
    a = torch.randn(M, K, device=dev).bfloat16()
    w = (torch.randn(N, K, device=dev) * 0.05).bfloat16()
    bias = torch.randn(N, device=dev).bfloat16()
    gate = torch.randn(N, device=dev).bfloat16()
    resid = torch.randn(M, N, device=dev).bfloat16()

    def run(cfg, rows=M, epi=_lib.EPI_BF16):
        o = resid[:rows].clone() if epi == _lib.EPI_GATE_RESID else torch.empty(rows, N, dtype=torch.bfloat16, device=dev)
        kw = dict(gate=gate, resid=o) if epi == _lib.EPI_GATE_RESID else {}
        ops.linear(a[:rows].contiguous(), w, bias, out=o, tile_cfg=cfg, epilogue=epi, **kw)
        torch.cuda.synchronize()
        return o.view(torch.int16).clone()

    for epi in (_lib.EPI_BF16, _lib.EPI_GATE_RESID):
        outs = {}
        for c in (2, 15, 13, 16, 17, -1):
            try:
                with _lib.tuning(gemm_splitk=0):  # -1: the automatic ONE-PASS choice (split-K associates K differently by design; its slices
                    outs[c] = run(c, epi=epi)     # follow one sample's groups: tests/test_engine_gpu.py::test_a_sample_does_not_depend_on_its_batch)
            except RuntimeError:  # a tile config that does not fit (N % 256, K-step) refuses: not part of the dispatcher's choice for this shape
                continue
        assert -1 in outs and len(outs) >= 2, f"configs that ran: {sorted(outs)}"
        ref = outs[-1]
        for c, o in outs.items():
            assert torch.equal(o, ref), f"bf16 tile config {c} differs from the automatic choice (epilogue {epi}, M={M} N={N} K={K}): {(o != ref).float().mean().item():.2e} of the elements"
        with _lib.tuning(gemm_splitk=0):  # the automatic ONE-PASS choice on a quarter of the rows: same bits as on all rows
            q = run(-1, rows=M // 4, epi=epi)
        assert torch.equal(q, ref[: M // 4]), "the one-pass result of a row depends on how many rows share its launch"


@pytest.mark.parametrize("B", [2, 4])
def test_attention_is_batch_invariant_at_thin_last_rounds(ops, dev, B):
    """Round 6: the balanced attention grid is planned PER SAMPLE and a batch is launched sample by sample when it is on, so
    at Flux-dev 768^2 (L = 2816: 33 tasks per XCD, the thin last round the DEFAULT tuning folds into the round in front of it) sample i of a
    batch gets exactly the bits it gets alone -- bf16 and fused-fp8 outputs.  Round 5 planned over B x heads x row blocks, which cut the same
    (head, row block) into different key pieces at B = 1 and B = 2 (<= 2.5e-3 apart).  flux_model.py:41-45 / 672-716: no cross-sample op."""
    H, L = 24, 2816
    assert ops.attention_plan(1, L, H) is not None and ops.attention_plan(1, L, H)["thin"]
    p1, pb = ops.attention_plan(1, L, H), ops.attention_plan(B, L, H)
    assert p1 == pb, "the plan must not depend on the batch"
    torch.manual_seed(83)
    q = torch.randn(B, H, L, 128).bfloat16()
    k = torch.randn(B, H, L, 128).bfloat16()
    v = torch.randn(B, H, L, 128).bfloat16()
    k = torch.where(k.abs() < 6.2e-5, torch.zeros_like(k), k)
    VT = _vt_layout(v, L)
    qd, kd, vd = q.to(dev), k.half().to(dev), VT.to(dev)
    s0, s1 = torch.tensor(3000.0, device=dev), torch.tensor(9000.0, device=dev)
    whole = ops.attention(qd, kd, vd)
    whole8 = ops.attention(qd, kd, vd, q_scale0=s0, q_scale1=s1, split=512)
    for i in range(B):
        one = ops.attention(qd[i:i + 1].contiguous(), kd[i:i + 1].contiguous(), vd[i:i + 1].contiguous())
        one8 = ops.attention(qd[i:i + 1].contiguous(), kd[i:i + 1].contiguous(), vd[i:i + 1].contiguous(), q_scale0=s0, q_scale1=s1, split=512)
        assert torch.equal(one[0].view(torch.int16), whole[i].view(torch.int16)), f"sample {i} of {B}: bf16 output differs from the sample alone"
        assert torch.equal(one8[0].view(torch.uint8), whole8[i].view(torch.uint8)), f"sample {i} of {B}: fp8 output differs from the sample alone"
    assert torch.isfinite(whole.float()).all()


@pytest.mark.parametrize("Ms", [(4608,), (2816,), (1000, 333), (4096, 512)])
def test_gemm_tile_config_20_matches_16(ops, dev, Ms):
    """Tile config 20 (round 6) = the one-wave-per-SIMD kernel with its four waves side by side along N (wave tile 224 x 64): 224 x 256 tiles, the
    exact fit of Flux-dev 1024^2 linear2 (M = 4608: 21 x 12 = 252 tiles = one round of the 256 CUs).  Same K loop, same MFMAs in the same order per
    output element: every byte must equal config 16's -- ragged last tiles (4608 = 20 x 224 + 128), two groups with their own weights, plain
    and ROW-PAIR activations / weights.                                           float8_quantize.py:284-292, flux_model.py:484"""
    from fluxmi import _lib

    torch.manual_seed(33)
    N, K = 3072, 15360 if len(Ms) == 1 else 8192
    one = torch.tensor(1.0, device=dev)
    a = [(torch.randn(M, K, device=dev) * 2).to(torch.float8_e5m2) for M in Ms]
    w = [(torch.randn(N, K, device=dev) * 0.5).to(torch.float8_e4m3fn) for _ in Ms]
    bias = torch.randn(N, device=dev).bfloat16()
    gate = torch.randn(N, device=dev).bfloat16()
    resid = [torch.randn(M, N, device=dev).bfloat16() for M in Ms]
    sar = torch.tensor(0.013, device=dev)
    even = all(M % 2 == 0 for M in Ms)
    ap = [ops.pair_rows(x.view(torch.uint8)).view(torch.float8_e5m2) for x in a] if even else None
    wp = [ops.pair_rows(x.view(torch.uint8)) for x in w]

    def launch(cfg, pairs=False):
        outs, groups = [], []
        for gi, M in enumerate(Ms):
            o = resid[gi].clone()
            outs.append(o)
            groups.append(ops.make_group((ap if pairs else a)[gi].data_ptr(), w[gi].data_ptr(), bias.data_ptr() if gi == 0 else None, sar.data_ptr(), one.data_ptr(),
                                         o.data_ptr(), M, K, N, gate=gate.data_ptr(), resid=o.data_ptr(), ldr=N, a_pairs=pairs,
                                         W_pairs=wp[gi].data_ptr() if pairs else None))
        ops.gemm_grouped(groups, N, K, True, E5M2, _lib.EPI_GATE_RESID, cfg)
        torch.cuda.synchronize()
        return [o.view(torch.int16).clone() for o in outs]

    ref = launch(16)
    for cfg in (20, 21):  # 21 = the same wave layout on 160-row tiles (768^2)
        for x, y in zip(ref, launch(cfg)):
            assert torch.equal(x, y), f"tile config {cfg} differs from config 16 (Ms = {Ms})"
        if even:
            for x, y in zip(ref, launch(cfg, pairs=True)):
                assert torch.equal(x, y), f"tile config {cfg} with row-pair operands differs from config 16 (Ms = {Ms})"
    for x in ref:
        assert torch.isfinite(x.view(torch.bfloat16).float()).all()


@pytest.mark.parametrize("epi_name", ["bf16", "gate_resid"])
def test_gemm_tile_config_17_bf16(ops, dev, epi_name):
    """Tile config 17 with bf16 operands (nn.Linear flows: Flux-schnell 256^2 linear1 at M = 512 -> 3 x 84 = 252 tiles of 192 rows instead of 168 of
    256; the text encoders): every output byte equals config 16's, ragged last tile (512 = 2 x 192 + 128) and a second group included, and the
    automatic dispatch agrees with both settings of fluxmi_tuning_t.gemm_tile192.                                   flux_model.py:471-473"""
    from fluxmi import _lib

    torch.manual_seed(37)
    N, K, Ms = 21504, 1024, [512, 100]
    epi = _lib.EPI_BF16 if epi_name == "bf16" else _lib.EPI_GATE_RESID
    a = [torch.randn(M, K, device=dev).bfloat16() for M in Ms]
    w = [(torch.randn(N, K, device=dev) * 0.05).bfloat16() for _ in Ms]
    bias = torch.randn(N, device=dev).bfloat16()
    gate = torch.randn(N, device=dev).bfloat16()
    resid = [torch.randn(M, N, device=dev).bfloat16() for M in Ms]

    def launch(cfg):
        outs, groups = [], []
        for gi, M in enumerate(Ms):
            o = resid[gi].clone()
            outs.append(o)
            kw = dict(gate=gate.data_ptr(), resid=o.data_ptr(), ldr=N) if epi == _lib.EPI_GATE_RESID else {}
            groups.append(ops.make_group(a[gi].data_ptr(), w[gi].data_ptr(), bias.data_ptr(), None, None, o.data_ptr(), M, K, N, **kw))
        ops.gemm_grouped(groups, N, K, False, E5M2, epi, cfg)
        torch.cuda.synchronize()
        return [o.view(torch.int16).clone() for o in outs]

    ref = launch(16)
    for cfg in (17, -1):
        for x, y in zip(ref, launch(cfg)):
            assert torch.equal(x, y), f"bf16 tile config {cfg} differs from config 16"
    with _lib.tuning(gemm_tile192=0):
        for x, y in zip(ref, launch(-1)):
            assert torch.equal(x, y)
    h = round_fp64_to_bf16(a[0].double().cpu() @ w[0].double().cpu().T + bias.double().cpu())
    if epi == _lib.EPI_BF16:
        assert_close_mag(ref[0].view(torch.bfloat16).cpu(), h, mag=accum_noise(a[0].cpu(), w[0].cpu(), 1.0), ulps=1.05, min_exact=0.98, what="bf16 cfg 16/17 vs fp64")


def test_gemm_persistent_quantising_paths_exhaustive(ops, dev):
    """The persistent kernel's table epilogue (table DMA issued inside the last K-step into ring slots 2 / 3, gather, transposition through
    the per-wave scratch) over EVERY bf16 input: A = 0, so h = bf16(0 * s + bias) is the bias pattern itself; the bias runs through all
    65536 bf16 patterns (NaNs and infinities included), 512 rows = two tiles per workgroup; every byte must equal table[h] with h taken
    from a plain bf16 launch of the same GEMM on the one-tile-per-workgroup kernel.      flux_model.py:301, float8_quantize.py:217-218"""
    from fluxmi import _lib

    M, N, K = 512, 65536, 512
    a = torch.zeros(M, K, dtype=torch.uint8, device=dev).view(torch.float8_e5m2)
    w = (torch.randn(N, K, device=dev) * 0.5).to(torch.float8_e4m3fn)
    bias = torch.arange(N, dtype=torch.int32, device=dev).to(torch.int16).view(torch.bfloat16)
    one = torch.tensor(1.0, device=dev)
    h = torch.zeros(M, N, dtype=torch.bfloat16, device=dev)
    g = ops.make_group(a.data_ptr(), w.data_ptr(), bias.data_ptr(), one.data_ptr(), one.data_ptr(), h.data_ptr(), M, K, N)
    ops.gemm_grouped([g], N, K, True, E5M2, _lib.EPI_BF16, 13)
    hbits = h.view(torch.int16).to(torch.int32) & 0xFFFF
    for scale in (1.0, 37.5, 9000.0):
        qs = torch.tensor(scale, device=dev)
        lut = ops.build_quant_lut(qs, E5M2, act=1)
        want = lut[hbits.long()]
        out = torch.full((M, N), 0x55, dtype=torch.uint8, device=dev)
        g8 = ops.make_group(a.data_ptr(), w.data_ptr(), bias.data_ptr(), one.data_ptr(), one.data_ptr(), out.data_ptr(), M, K, N,
                            q_scale=qs.data_ptr(), q_lut=lut.data_ptr())
        ops.gemm_grouped([g8], N, K, True, E5M2, _lib.EPI_GELU_QUANT, 18)
        bad = (out != want)
        assert not bad.any(), (f"scale {scale}: {int(bad.sum())} bytes differ from the table; first patterns "
                               f"{[hex(int(v)) for v in hbits[bad][:8].tolist()]} rows {torch.nonzero(bad)[:4, 0].tolist()}")


@pytest.mark.parametrize("cfg", [2, 13, 16, 17, 18, -1])
def test_gemm_row_pair_activations(ops, dev, cfg):
    """ABI 5 (round 6): fluxmi_gemm_group_t.a_pairs -- the fp8 A operand stored as [M/2][K/64][2][64] (ops.pair_rows), what the engine's
    LayerNorm / attention / GELU epilogues write in fused mode -- and c8_pairs -- the fp8 output of the quantising epilogues written in that
    layout for the next linear.  Same values at other addresses: every tile config that honours the flags must give the bits of the plain
    launch (bf16 / gate*y+x outputs identical; unpaired fp8 outputs identical), two groups with ragged-free even M, table and computed
    GELU; the generic and split-K kernels refuse a flagged group.             float8_quantize.py:272-296 (layout-only: no arithmetic changes)"""
    from fluxmi import _lib

    torch.manual_seed(41)
    N, K = 3072, (8192 if cfg in (16, 17) else 3072)
    Ms = (640, 1022) if cfg != 18 else (4096, 1024)  # the persistent kernel takes launches of more than 256 tiles
    one = torch.tensor(1.0, device=dev)
    sar = torch.tensor(0.02, device=dev)
    qs = torch.tensor(37.5, device=dev)
    lut = ops.build_quant_lut(qs, E5M2, act=1)
    a = [(torch.randn(M, K, device=dev) * 2).to(torch.float8_e5m2) for M in Ms]
    ap = [ops.pair_rows(x.view(torch.uint8)).view(torch.float8_e5m2) for x in a]
    w = [(torch.randn(N, K, device=dev) * 0.5).to(torch.float8_e4m3fn) for _ in Ms]
    bias = torch.randn(N, device=dev).bfloat16()
    gate = torch.randn(N, device=dev).bfloat16()
    resid = [torch.randn(M, N, device=dev).bfloat16() for M in Ms]

    def launch(epi, pairs_in, pairs_out, table):
        outs, groups = [], []
        for gi, M in enumerate(Ms):
            src = ap[gi] if pairs_in else a[gi]
            if epi == _lib.EPI_GATE_RESID:
                o = resid[gi].clone()
                kw = dict(gate=gate.data_ptr(), resid=o.data_ptr(), ldr=N)
            elif epi == _lib.EPI_GELU_QUANT:
                o = torch.zeros(M, N, dtype=torch.uint8, device=dev)
                kw = dict(q_scale=qs.data_ptr(), q_lut=lut.data_ptr() if table else None)
            else:
                o = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
                kw = {}
            outs.append(o)
            groups.append(ops.make_group(src.data_ptr(), w[gi].data_ptr(), bias.data_ptr(), sar.data_ptr(), one.data_ptr(), o.data_ptr(), M, K, N,
                                         a_pairs=pairs_in, c8_pairs=pairs_out, **kw))
        ops.gemm_grouped(groups, N, K, True, E5M2, epi, cfg)
        torch.cuda.synchronize()
        if pairs_out:  # back to plain rows for the comparison
            outs = [ops.unpair_rows(o) for o in outs]
        return [o.view(torch.int16 if o.dtype == torch.bfloat16 else torch.uint8).clone() for o in outs]

    epis = [_lib.EPI_GATE_RESID] if cfg in (16, 17) else [_lib.EPI_BF16, _lib.EPI_GATE_RESID, _lib.EPI_GELU_QUANT]
    for epi in epis:
        for table in ((True,) if cfg == 18 else (False, True)) if epi == _lib.EPI_GELU_QUANT else (False,):
            if table and cfg not in (13, 18, -1):
                continue  # the table epilogue exists in the 256 x 256 LDS-epilogue kernels only
            ref = launch(epi, False, False, table)
            got = launch(epi, True, epi == _lib.EPI_GELU_QUANT, table)
            for x, y in zip(ref, got):
                assert torch.equal(x, y), f"tile config {cfg}, epilogue {epi}, table {table}: row-pair activations change the result ({(x != y).float().mean().item():.2e} of the elements)"
            if epi == _lib.EPI_GELU_QUANT:  # mixed: plain A, paired output
                for x, y in zip(ref, launch(epi, False, True, table)):
                    assert torch.equal(x, y)
    if cfg == -1:
        g = ops.make_group(ap[0].data_ptr(), w[0].data_ptr(), bias.data_ptr(), sar.data_ptr(), one.data_ptr(), resid[0].data_ptr(), Ms[0], K, N, a_pairs=True)
        with pytest.raises(RuntimeError, match="row-pair"):
            ops.gemm_grouped([g], N, K, True, E5M2, _lib.EPI_BF16, 100)


def test_quantising_epilogue_computed_vs_table_exhaustive(ops, dev):
    """is the 64 KiB table (fluxmi_gemm_group_t.q_lut, built by build_qlut_kernel) bit-identical to the epilogue the
    kernels COMPUTE when no table is given?  Exhaustive over all 65536 bf16 inputs (A = 0, bias = every pattern) for every kernel that has a
    computed GELU + quantise epilogue (tile configs 2, 13, 16; the persistent kernel takes the table or refuses), at three scales; both are
    compared with the oracle's torch chain (F.gelu(tanh) -> bf16 -> x scale -> bf16 -> clamp -> e5m2: flux_model.py:301,
    float8_quantize.py:217-218,274-276).  MEASURED (profiles/r06_qlut_vs_computed.txt): the table equals the oracle on every finite pattern
    but the cliff below; the computed epilogues equal the table on all but ONE of 65536 patterns (hipcc contracts the GELU polynomial into
    different fma's inside the GEMM kernels than inside build_qlut_kernel) -- "same helpers, so bit-identical" was off by that one pattern;
    the table is the more faithful path and it is the default.  The cliff: for -5.16 <= h <= -5.06, 1 + tanh(u) is 0 or 2^-24 in fp32
    depending on the tanh implementation (torch CPU: 0 -> gelu = -0; the device: 2^-24 -> -1.5e-7); at scale 9000 that is fp8 byte 0x96
    against 0x80.  Gates: >= 99.9 % of the finite patterns exact and nothing beyond 1 fp8 ulp outside the cliff, for the table and for every
    computed epilogue; computed == table on >= 99.99 %; the table agrees with the oracle at least as often as any computed epilogue."""
    from fluxmi import _lib

    M, N, K = 512, 65536, 512
    a = torch.zeros(M, K, dtype=torch.uint8, device=dev).view(torch.float8_e5m2)
    w = (torch.randn(N, K, device=dev) * 0.5).to(torch.float8_e4m3fn)
    bias = torch.arange(N, dtype=torch.int32, device=dev).to(torch.int16).view(torch.bfloat16)
    one = torch.tensor(1.0, device=dev)
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    ok_in = torch.isfinite(bits.float())  # +-inf / NaN inputs: F.gelu(-inf) is NaN in torch and -0 here; no finite model produces them
    cliff = (bits.float() >= -5.2) & (bits.float() <= -5.0)

    def check(x, what):
        dd = f8_ulp_diff(x.view(torch.float8_e5m2), ref.view(torch.float8_e5m2))
        far = torch.nonzero((dd > 1) & ok_in & ~cliff).flatten()
        assert len(far) == 0, f"{what}: beyond 1 fp8 ulp outside the tanh cliff: " + ", ".join(
            f"h={bits[i].item():.6g} got 0x{int(x[i]):02x} oracle 0x{int(ref[i]):02x}" for i in far[:8])
        exact = (x[ok_in] == ref[ok_in]).float().mean().item()
        assert exact >= 0.999, f"{what}: exact on {exact:.6f} of the finite patterns"
        return exact, int(((dd > 1) & ok_in & cliff).sum())

    for scale in (1.0, 37.5, 9000.0):
        qs = torch.tensor(scale, device=dev)
        lut = ops.build_quant_lut(qs, E5M2, act=1).cpu()
        ref = fo.to_fp8_saturated(F.gelu(bits, approximate="tanh"), torch.tensor(scale), 57344.0).to(torch.float8_e5m2).view(torch.uint8)
        e_t, c_t = check(lut, "table")
        line = [f"scale {scale}: table == oracle on {e_t:.6f} of the finite patterns ({c_t} cliff patterns beyond 1 ulp)"]
        worst = 1.0
        for cfg in (2, 13, 16):
            out = torch.full((M, N), 0x55, dtype=torch.uint8, device=dev)
            g8 = ops.make_group(a.data_ptr(), w.data_ptr(), bias.data_ptr(), one.data_ptr(), one.data_ptr(), out.data_ptr(), M, K, N, q_scale=qs.data_ptr())
            ops.gemm_grouped([g8], N, K, True, E5M2, _lib.EPI_GELU_QUANT, cfg)
            rows = out.cpu()
            assert (rows == rows[0:1]).all(), f"cfg {cfg}: rows of one column differ"
            got = rows[0]
            e_c, c_c = check(got, f"computed epilogue of tile config {cfg}")
            same_t = (got[ok_in] == lut[ok_in]).float().mean().item()
            n_diff = int((got[ok_in] != lut[ok_in]).sum())
            line.append(f"cfg {cfg}: computed == table on all but {n_diff}, == oracle {e_c:.6f}")
            assert same_t >= 0.9999
            worst = min(worst, e_c)
        print("; ".join(line))
        assert e_t >= worst - 1e-9


@pytest.mark.parametrize("cfg", [2, 13, 16, 100])
def test_gemm_epilogues(ops, dev, cfg):
    """K8/K9/K2 fused epilogues == the reference's eager chain applied to the GEMM's own bf16 output."""
    from fluxmi import _lib

    M, N, K = 384, 1024, 256
    a8, w8, sar, sbr, bias = make_f8_problem(M, N, K, E5M2, seed=11)
    d = lambda t: t.to(dev)
    h = ops.linear(d(a8), d(w8), d(bias), d(sar), d(sbr), tile_cfg=cfg).cpu()  # bf16(acc*s+bias)
    qs = torch.tensor(37.5, dtype=torch.float32)
    # GELU + quantise                                                     flux_model.py:301 + float8_quantize.py:274-276
    ref = fo.to_fp8_saturated(F.gelu(h, approximate="tanh"), qs, 57344.0).to(torch.float8_e5m2)
    got = ops.linear(d(a8), d(w8), d(bias), d(sar), d(sbr), epilogue=_lib.EPI_GELU_QUANT, q_scale=d(qs), tile_cfg=cfg)
    assert_f8_close(got, ref, max_ulp=1, min_exact=0.999, what="gelu+quant")
    # gate * y + x                                                        flux_model.py:387-388
    g = torch.Generator().manual_seed(3)
    gate = torch.randn(N, generator=g).bfloat16()
    resid = torch.randn(M, N, generator=g).bfloat16()
    ref = resid + gate * h
    got = ops.linear(d(a8), d(w8), d(bias), d(sar), d(sbr), epilogue=_lib.EPI_GATE_RESID, gate=d(gate), resid=d(resid), tile_cfg=cfg)
    assert torch.equal(got.cpu(), ref), f"gate-resid: max ulp {ulp_diff(got, ref).max().item()}"
    # in place on the residual buffer
    r2 = d(resid).clone()
    ops.linear(d(a8), d(w8), d(bias), d(sar), d(sbr), epilogue=_lib.EPI_GATE_RESID, gate=d(gate), resid=r2, out=r2, tile_cfg=cfg)
    assert torch.equal(r2.cpu(), ref)
    # split: qkv part bf16, mlp part gelu+quant into a wider buffer at a column offset   flux_model.py:471-480
    split = 512
    out2 = torch.zeros(M, 128 + (N - split), dtype=torch.float8_e5m2, device=dev)
    got = ops.linear(d(a8), d(w8), d(bias), d(sar), d(sbr), epilogue=_lib.EPI_SPLIT, q_scale=d(qs), out2=out2, split_n=split,
                     c2_col0=128, tile_cfg=cfg)
    assert torch.equal(got.cpu(), h[:, :split])
    ref = fo.to_fp8_saturated(F.gelu(h[:, split:], approximate="tanh"), qs, 57344.0).to(torch.float8_e5m2)
    assert_f8_close(out2[:, 128:], ref, max_ulp=1, min_exact=0.999, what="split gelu+quant")
    assert (out2[:, :128].cpu().view(torch.uint8) == 0).all()


def test_gemm_grouped(ops, dev):
    """txt+img streams (different weights, different M incl. a ragged one) in one launch."""
    from fluxmi import _lib

    N, K = 512, 256
    probs = [make_f8_problem(M, N, K, E5M2, seed=100 + M) for M in (64, 333, 256)]
    outs, groups, keep = [], [], []
    for a8, w8, sar, sbr, bias in probs:
        t = [x.to(dev) for x in (a8, w8, sar, sbr, bias)]
        o = torch.empty(a8.shape[0], N, dtype=torch.bfloat16, device=dev)
        keep.append(t)
        outs.append(o)
        groups.append(ops.make_group(t[0].data_ptr(), t[1].data_ptr(), t[4].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                                     o.data_ptr(), a8.shape[0], K, N))
    for cfg in (2, 13):
        for o in outs:
            o.zero_()
        ops.gemm_grouped(groups, N, K, True, E5M2, _lib.EPI_BF16, cfg)
        for (a8, w8, sar, sbr, bias), o in zip(probs, outs):
            ref = round_fp64_to_bf16(fo.scaled_mm_fp64(a8, w8, sar, sbr, bias))
            assert_close_mag(o, ref, mag=accum_noise(a8, w8, sar * sbr), ulps=1, min_exact=0.98, what=f"grouped cfg={cfg} M={a8.shape[0]}")


@pytest.mark.parametrize("B", [1, 3, 8])
def test_gemv(ops, dev, B):
    """K10: Modulation / MLPEmbedder skinny linears (flux_model.py:251-257,154-155)."""
    torch.manual_seed(7)
    K, N = 768, 200
    x = torch.randn(B, K).bfloat16()
    w = (torch.randn(N, K) * 0.05).bfloat16()
    bias = torch.randn(N).bfloat16()
    d = lambda t: t.to(dev)
    # fp8 weights, SiLU prologue
    st = fo.F8LinearState(w, bias)
    ref = st(F.silu(x))  # first calibration call fixes the scale from this input
    out = ops.gemv(d(x), d(st.float8_data), d(bias), d(st.input_scale), d(st.input_scale_reciprocal), d(st.scale_reciprocal),
                   pre_silu=True)
    ref64 = round_fp64_to_bf16(fo.scaled_mm_fp64(st.quantize_input(F.silu(x)), st.float8_data, st.input_scale_reciprocal,
                                                 st.scale_reciprocal, bias))
    x8 = st.quantize_input(F.silu(x))
    noise = accum_noise(x8, st.float8_data, st.input_scale_reciprocal * st.scale_reciprocal)
    assert_close_mag(out, ref64, mag=noise, ulps=1, min_exact=0.98, what="gemv fp8")
    assert_close_mag(out, ref, mag=noise, ulps=1, min_exact=0.98, what="gemv fp8 vs scaled_mm")
    # bf16 weights, no prologue
    out = ops.gemv(d(x), d(w), d(bias))
    ref = round_fp64_to_bf16(x.double() @ w.double().T + bias.double())
    assert_close_mag(out, ref, mag=accum_noise(x, w, 1.0), ulps=1, min_exact=0.98, what="gemv bf16")


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["stream", "stream_2wg", "row_per_wave"])
@pytest.mark.parametrize("L,Lt", [(40, 12), (42, 13), (1300, 500)])
@pytest.mark.parametrize("H", [256, 3072])
def test_ln_modulate(ops, dev, H, L, Lt, variant):
    """K4(+K2): (1+scale)*LayerNorm(x)+shift with the reference's bf16 rounding points (flux_model.py:367-368).
    (42, 13): a workgroup's rows straddle the txt|img split and the batch boundary (the rows that do not belong to the
    workgroup's LDS-staged table take their modulation vectors from global memory); (1300, 500): 256 workgroups with 10-11 rows each,
    i.e. the streaming kernel's prefetch loop runs (every wave owns two rows, some a single one).
    Both kernels: the streaming one (default, fluxmi_tuning_t.ln_variant = 2; 3 = its grid at two workgroups per CU) and the
    one-wave-per-row one (1)."""
    from fluxmi import _lib

    with _lib.tuning(ln_variant={"stream": 2, "stream_2wg": 3, "row_per_wave": 1}[variant]):
        _ln_modulate_body(ops, dev, H, L, Lt)


def _ln_modulate_body(ops, dev, H, L, Lt):
    torch.manual_seed(9)
    B = 2
    x = (torch.randn(B, L, H) * 2 + 0.3).bfloat16()
    mods = (torch.randn(B, 4 * H) * 0.5).bfloat16()  # txt shift|scale, img shift|scale, row stride 4H
    sh0, sc0, sh1, sc1 = mods[:, :H], mods[:, H:2 * H], mods[:, 2 * H:3 * H], mods[:, 3 * H:]
    ln = F.layer_norm(x, (H,), eps=1e-6)
    ref = torch.empty_like(x)
    ref[:, :Lt] = (1 + sc0[:, None]) * ln[:, :Lt] + sh0[:, None]
    ref[:, Lt:] = (1 + sc1[:, None]) * ln[:, Lt:] + sh1[:, None]
    md = mods.to(dev)
    v = lambda a, b: md[:, a * H:b * H]
    got = ops.ln_modulate(x.to(dev), v(0, 1), v(1, 2), v(2, 3), v(3, 4), split=Lt)
    mag = torch.empty(B, L, H)
    mag[:, :Lt] = ((1 + sc0[:, None]) * ln[:, :Lt]).float().abs() + sh0[:, None].float().abs()
    mag[:, Lt:] = ((1 + sc1[:, None]) * ln[:, Lt:]).float().abs() + sh1[:, None].float().abs()
    # three chained bf16 roundings: a 1-ulp flip of LN(x) (summation order of mean/var) is amplified by (1+scale) <= ~3
    assert_close_mag(got, ref, mag=mag, ulps=2, min_exact=0.999, what="ln_modulate bf16")
    q0, q1 = torch.tensor(900.0), torch.tensor(20000.0)
    refq = torch.empty(B, L, H, dtype=torch.float8_e5m2)
    refq[:, :Lt] = fo.to_fp8_saturated(ref[:, :Lt], q0, 57344.0).to(torch.float8_e5m2)
    refq[:, Lt:] = fo.to_fp8_saturated(ref[:, Lt:], q1, 57344.0).to(torch.float8_e5m2)
    gotq = ops.ln_modulate(x.to(dev), v(0, 1), v(1, 2), v(2, 3), v(3, 4), split=Lt, q_scale0=q0.to(dev), q_scale1=q1.to(dev))
    assert_f8_close(gotq, refq, max_ulp=1, min_exact=0.999, what="ln_modulate fp8")


def test_act_tables(ops, dev):
    """K9/K10: GELU(tanh) and SiLU over every finite bf16 input vs ATen's CPU kernels."""
    x = all_bf16()
    x = x[torch.isfinite(x)]
    x = x[: (x.numel() // 8) * 8].reshape(-1, 8)
    g = ops.act(x.to(dev), 0)
    # results below 1e-4 come out of the 1+tanh / 1+exp cancellation: compare those on an absolute 1e-4*2^-7 scale
    assert_close_mag(g, F.gelu(x, approximate="tanh"), mag=1e-4, ulps=1, min_exact=0.999, what="gelu table")
    s = ops.act(x.to(dev), 1)
    assert_close_mag(s, F.silu(x), mag=1e-4, ulps=1, min_exact=0.999, what="silu table")


def test_gate_residual_add_euler(ops, dev):
    torch.manual_seed(4)
    B, L, H = 2, 24, 256
    x, y = torch.randn(B, L, H).bfloat16(), torch.randn(B, L, H).bfloat16()
    gate = torch.randn(B, H).bfloat16()
    assert torch.equal(ops.gate_residual(x.to(dev), y.to(dev), gate.to(dev)).cpu(), x + gate[:, None] * y)
    assert torch.equal(ops.add(x.to(dev), y.to(dev)).cpu(), x + y)
    dt = 0.9762182831764221 - 0.9884144067764282
    img = x.to(dev).clone()
    ops.euler_(img, y.to(dev), dt)
    assert torch.equal(img.cpu(), x + dt * y)


def test_rope_table_and_timestep_embedding(ops, dev):
    """K13/K12 vs flux_model.py:49-57,82-92 and :95-116."""
    img_ids, txt_ids = fo.make_ids(2, 16, 16, 24, torch.bfloat16)
    ids = torch.cat((txt_ids, img_ids), dim=1)
    ref = fo.rope_table(ids, [16, 56, 56], 10000, torch.bfloat16)  # [B,1,L,64,2,2]
    pe = ops.rope_table(ids.to(dev), [16, 56, 56], 10000).cpu()
    assert_bf16_close(pe[..., 0], ref[:, 0, :, :, 0, 0], 1, 0.999, what="rope cos")
    assert_bf16_close(pe[..., 1], ref[:, 0, :, :, 1, 0], 1, 0.999, what="rope sin")
    ts = fo.get_schedule(28, 4096)
    t = torch.tensor(ts[:-1] + [3.5], dtype=torch.float32).bfloat16()  # the 28 bf16-rounded schedule points + guidance
    ref = fo.timestep_embedding(t, 256).bfloat16()
    got = ops.timestep_embedding(t.to(dev), ops.timestep_freqs_host().to(dev))
    assert_bf16_close(got, ref, max_ulp=1, min_exact=0.995, what="timestep embedding")


@pytest.mark.parametrize("L,Lt", [(128, 32), (200, 72)])
def test_qkv_rope(ops, dev, L, Lt):
    """K5+K6+K11: split + QK RMSNorm (fp32) + RoPE (bf16 arithmetic) + relayout (flux_model.py:351-354,158-176,60-65)."""
    torch.manual_seed(6)
    B, H = 2, 3
    extra = 64  # qkv lives inside a wider row (SingleStreamBlock.linear1 output)
    qkv_full = torch.randn(B, L, 3 * H * 128 + extra).bfloat16()
    qkv = qkv_full[..., : 3 * H * 128]
    s = [(1 + 0.1 * torch.randn(128)).bfloat16() for _ in range(4)]  # txt q,k ; img q,k
    side = int(math.isqrt(L - Lt)) if int(math.isqrt(L - Lt)) ** 2 == L - Lt else None
    img_ids = torch.zeros(B, L - Lt, 3, dtype=torch.bfloat16)
    img_ids[..., 1] = (torch.arange(L - Lt) // 8).bfloat16()
    img_ids[..., 2] = (torch.arange(L - Lt) % 8).bfloat16()
    ids = torch.cat((torch.zeros(B, Lt, 3, dtype=torch.bfloat16), img_ids), 1)
    pe6 = fo.rope_table(ids, [16, 56, 56], 10000, torch.bfloat16)
    q, k, v = fo.split_heads(qkv, H)
    qn = torch.cat((fo.rms_norm(q[:, :, :Lt], s[0]), fo.rms_norm(q[:, :, Lt:], s[2])), 2)
    kn = torch.cat((fo.rms_norm(k[:, :, :Lt], s[1]), fo.rms_norm(k[:, :, Lt:], s[3])), 2)
    q_ref, k_ref = fo.apply_rope(qn, kn, pe6)
    pe = torch.stack((pe6[:, 0, :, :, 0, 0], pe6[:, 0, :, :, 1, 0]), -1).contiguous()  # exact table -> isolates this kernel
    d = lambda t: t.to(dev)
    Q, K, VT = ops.qkv_rope(d(qkv_full)[..., : 3 * H * 128], d(pe), d(s[0]), d(s[1]), d(s[2]), d(s[3]), split=Lt, heads=H)
    assert_bf16_close(Q, q_ref, max_ulp=1, min_exact=0.999, what="Q")
    assert_bf16_close(K, k_ref, max_ulp=1, min_exact=0.999, what="K")
    # V^T with the bit2<->bit3 key permutation inside every 16-key group, zero padded to Lp
    Lp = VT.shape[-1]
    pos = torch.arange(Lp)
    j = pos % 16
    key = (pos // 16) * 16 + ((j & 3) | (((j >> 2) & 1) << 3) | (((j >> 3) & 1) << 2))
    vpad = torch.zeros(B, H, Lp, 128, dtype=torch.bfloat16)
    vpad[:, :, :L] = v
    assert torch.equal(VT.cpu(), vpad[:, :, key].transpose(-1, -2))


@pytest.mark.parametrize("B,H,L,Lt", [(1, 2, 320, 64), (2, 1, 200, 40), (1, 2, 33, 8), (1, 1, 97, 32), (1, 1, 4608, 512)])
def test_attention(ops, dev, B, H, L, Lt):
    """K7: softmax(QK^T/sqrt(128))V vs fp64 (flux_model.py:41-45); bf16 and fused-fp8 outputs."""
    torch.manual_seed(8)
    q = torch.randn(B, H, L, 128).bfloat16()
    k = torch.randn(B, H, L, 128).bfloat16()
    v = torch.randn(B, H, L, 128).bfloat16()
    q[:, :, 5] *= 4.0  # a peaky row: exercises the running-max rescale
    k[:, :, L // 2] *= 3.0
    ref, A = ar.attention_ref64(q, k, v)
    Lp = (L + 63) // 64 * 64
    pos = torch.arange(Lp)
    j = pos % 16
    key = (pos // 16) * 16 + ((j & 3) | (((j >> 2) & 1) << 3) | (((j >> 3) & 1) << 2))
    vpad = torch.zeros(B, H, Lp, 128, dtype=torch.bfloat16)
    vpad[:, :, :L] = v
    VT = vpad[:, :, key].transpose(-1, -2).contiguous()
    d = lambda t: t.to(dev)
    out = ops.attention(d(q), d(k), d(VT)).cpu()
    ar.assert_attention_close(out, q, k, v, False, f"test_attention B={B} H={H} L={L} bf16 K")
    # the framework's SDPA in fp32 is the same function as the fp64 reference (fp32 roundoff on scores up to ~100: 1e-4 relative with room),
    # so the gate above holds against it as well
    sdpa = F.scaled_dot_product_attention(q.float(), k.float(), v.float()).transpose(1, 2).reshape(B, L, H * 128)
    assert ((sdpa.double() - ref).abs() <= 1e-4 * (ref.abs() + A)).all()
    # fused quantised output, two scales split at Lt                      float8_quantize.py:274-276
    s0, s1 = torch.tensor(3000.0), torch.tensor(9000.0)
    got = ops.attention(d(q), d(k), d(VT), q_scale0=d(s0), q_scale1=d(s1), split=Lt).cpu()
    deq = torch.cat((got[:, :Lt].float() / s0, got[:, Lt:].float() / s1), 1)
    # e5m2 has 2 mantissa bits: relative step 2^-2 -> half-step 12.5 %; compare against the quantised bf16 output
    refq = torch.cat((fo.to_fp8_saturated(out[:, :Lt], s0, 57344.0).to(torch.float8_e5m2).float() / s0,
                      fo.to_fp8_saturated(out[:, Lt:], s1, 57344.0).to(torch.float8_e5m2).float() / s1), 1)
    assert torch.equal(deq, refq), f"fp8 attention output differs from quantise(bf16 output): {(deq != refq).float().mean().item()}"
    # fp16 K (the engine's operand format): the folded kernel
    k16 = torch.where(k.abs() < 6.2e-5, torch.zeros_like(k), k)  # below fp16's normal range a bf16 value is not exact in fp16
    out4 = ops.attention(d(q), d(k16.half()), d(VT)).cpu()
    ar.assert_attention_close(out4, q, k16, v, True, f"test_attention B={B} H={H} L={L} fp16 K")
    got4 = ops.attention(d(q), d(k16.half()), d(VT), q_scale0=d(s0), q_scale1=d(s1), split=Lt).cpu()
    refq4 = torch.cat((fo.to_fp8_saturated(out4[:, :Lt], s0, 57344.0).to(torch.float8_e5m2).float(),
                       fo.to_fp8_saturated(out4[:, Lt:], s1, 57344.0).to(torch.float8_e5m2).float()), 1)
    assert torch.equal(got4.float(), refq4), "fp8 output (fp16 K) differs from quantise(its bf16 output)"


def _vt_layout(v, L, Lp=None, fill=None):
    """V^T in the attention kernels' layout: transposed, key order inside every 16-key group with bit2 <-> bit3 swapped, zero padded to Lp
    (default: the next multiple of 64); fill: a bf16 [B, H, Lp, 128] tensor whose rows >= L replace the zero padding"""
    B, H = v.shape[:2]
    Lp = (L + 63) // 64 * 64 if Lp is None else Lp
    pos = torch.arange(Lp)
    j = pos % 16
    key = (pos // 16) * 16 + ((j & 3) | (((j >> 2) & 1) << 3) | (((j >> 3) & 1) << 2))
    vpad = torch.zeros(B, H, Lp, 128, dtype=torch.bfloat16) if fill is None else fill.clone()
    vpad[:, :, :L] = v
    return vpad[:, :, key].transpose(-1, -2).contiguous()


@pytest.mark.parametrize("L", [448, 1100, 4608])
def test_attention_deferred_rescale_branch(ops, dev, L):
    """The kernel rescales O / l / the pending P tile only when a row max grew by more than 2^8 (guide T13).  The branch is rare on
    random data, so it is FORCED: key rows are spiked against chosen query rows so that the row max jumps by far more than the threshold
    at chosen tiles (first tile, an odd tile, an even tile, the last tile; both 32-key halves of a tile), some rows several times; every
    row of the full tensor is checked against fp64, and the builds -- bf16 K (unfolded) and fp16 K (folded: softmax scale in Q, running
    max in the accumulator init; the engine's default), each with deferred and with exact running max (fluxmi_tuning_t.attn_var = 2) --
    must agree to rounding.  The fused fp8 output through the regrouped 16-byte stores must equal the 4-byte stores bit for bit."""
    from fluxmi import _lib

    torch.manual_seed(81)
    B, H = 1, 2
    q = torch.randn(B, H, L, 128).bfloat16()
    k = torch.randn(B, H, L, 128).bfloat16()
    v = torch.randn(B, H, L, 128).bfloat16()
    nt = (L + 63) // 64
    # scores are q.k/sqrt(128)*log2(e) ~ N(0, 1.44) in the exp2 domain; a key equal to +7 x a query row scores ~ 7*128/11.3*1.44 = 114
    for t_i, (row, tile, gain) in enumerate([(3, 0, 5.0), (3, 3, 7.0), (3, nt - 1, 9.0), (40, 2, 6.0), (41, nt - 2, 6.0), (L - 1, 1, 8.0),
                                             (L // 2, nt // 2, 6.0), (L // 2, nt // 2 + 1, 8.0)]):
        key = min(tile * 64 + 5 + t_i + 32 * (t_i & 1), L - 1)
        k[:, :, key] = (q[:, :, row].float() * gain).bfloat16()
    k = torch.where(k.abs() < 6.2e-5, torch.zeros_like(k), k)  # below fp16's normal range a bf16 value is not exact in fp16 (engine: |k| ~ 1)
    assert torch.equal(k.half().float(), k.float())
    ref_A = ar.attention_ref64(q, k, v)
    ref = ref_A[0]
    # the exact-max builds round a pending P tile a second time whenever a row max grows: attention_model(exact=True) has that rounding point
    gates = {(var, f16): ar.attention_gate(q, k, v, f16, exact=var == 2, ref_A=ref_A) for var in (0, 2) for f16 in (False, True)}
    VT = _vt_layout(v, L)
    d = lambda t: t.to(dev)
    outs = {}
    variants = (("deferred", 0, False), ("exact", 2, False), ("fold", 0, True), ("fold_exact", 2, True))
    s0, s1 = torch.tensor(3000.0), torch.tensor(9000.0)
    for name, var, f16 in variants:
        kd = d(k.half() if f16 else k)
        with _lib.tuning(attn_var=var, attn_abl=0):
            outs[name] = ops.attention(d(q), kd, d(VT)).cpu()
            # fused fp8 output: regrouped 16-byte stores == 4-byte stores
            f8_new = ops.attention(d(q), kd, d(VT), q_scale0=d(s0), q_scale1=d(s1), split=L // 3).cpu()
        ar.assert_attention_close(outs[name], q, k, v, f16, f"deferred_rescale L={L} {name}", gate=gates[var, f16])
        with _lib.tuning(attn_var=var, attn_abl=8):
            f8_old = ops.attention(d(q), kd, d(VT), q_scale0=d(s0), q_scale1=d(s1), split=L // 3).cpu()
        assert torch.equal(f8_new.view(torch.uint8), f8_old.view(torch.uint8)), f"{name}: fp8 store variants differ"
    for name, var, f16 in variants[1:]:  # two builds inside their gates are within the sum of the two limits of each other, element by element
        lim = ar.MARGIN * (max(1.0, gates[0, False]["r_model"]) + max(1.0, gates[var, f16]["r_model"])) * gates[0, False]["bound"]
        dd = (outs["deferred"].double() - outs[name].double()).abs()
        assert (dd <= lim).all(), f"deferred vs {name}: {(dd / lim.clamp_min(1e-300)).max().item():.3f} x the two gates"
    e = lambda n: (outs[n].double() - ref).abs().max().item()
    r = lambda n: ((outs[n].double() - ref).norm() / ref.norm()).item()
    # the fold must not cost accuracy (a bf16 fold did: rel-L2 1.8e-3 -> 3.3e-3 on these inputs)
    assert r("fold") <= 1.15 * r("deferred") + 1e-4 and r("fold_exact") <= 1.15 * r("exact") + 1e-4, (r("fold"), r("deferred"), r("fold_exact"), r("exact"))
    same = (outs["deferred"] == outs["exact"]).float().mean().item()
    same_f = (outs["deferred"] == outs["fold"]).float().mean().item()
    print(f"L={L}: max |err| vs fp64 deferred {e('deferred'):.2e} / exact {e('exact'):.2e} / fold {e('fold'):.2e} / fold_exact {e('fold_exact'):.2e}; "
          f"rel-L2 deferred {r('deferred'):.3e} fold {r('fold'):.3e} exact {r('exact'):.3e} fold_exact {r('fold_exact'):.3e}; "
          f"deferred == exact on {same:.4f}, == fold on {same_f:.4f} of the outputs")


@pytest.mark.parametrize("B,H,L", [(1, 8, 1100), (1, 24, 1536), (1, 24, 2816), (1, 24, 4608), (2, 24, 4608)])
def test_attention_balanced_grid(ops, dev, B, H, L):
    """fluxmi_tuning_t.attn_split (round 5; forced here, the default takes it for thin last rounds such as L = 2816): the workgroups of the
    last, partial round are replaced by PIECES of their tasks' key range
    (fluxmi_attention_plan); every piece keeps its own running max / row sum / O and the last arriver of a task merges them.  Checks:
    the plan is on for these shapes; bf16 and fused-fp8 outputs of the balanced grid == one workgroup per task up to fp32 summation order
    (same gates as between the other kernel builds); repeated launches are bit-identical (the merge order is fixed, not arrival order) and
    leave the arrival counters at zero (a second, third launch gives the same bits); key rows spiked in different pieces give row maxima
    that differ by far more than the deferred-rescale threshold between the pieces of a task; the small shape is also checked against fp64
    (sequence not a multiple of 64: the last piece masks its partial tile).                                     flux_model.py:41-45"""
    from fluxmi import _lib

    plan = ops.attention_plan(B, L, H)
    assert plan is not None and any(p["np"] > 1 for p in plan["pieces"])
    torch.manual_seed(82)
    q = torch.randn(B, H, L, 128).bfloat16()
    k = torch.randn(B, H, L, 128).bfloat16()
    v = torch.randn(B, H, L, 128).bfloat16()
    nt = (L + 63) // 64
    # spikes: every query row of the LAST row block of the last head (a leftover task) sees its maximum in another piece
    for t_i, (row, tile, gain) in enumerate([(L - 1, 0, 6.0), (L - 2, nt // 2, 8.0), (L - 3, nt - 1, 9.0), (L - 200, nt // 3, 7.0), (L - 201, 2 * nt // 3, 7.0)]):
        k[:, H - 1, min(tile * 64 + 7 + t_i, L - 1)] = (q[:, H - 1, row].float() * gain).bfloat16()
    k = torch.where(k.abs() < 6.2e-5, torch.zeros_like(k), k)
    VT = _vt_layout(v, L)
    d = lambda t: t.to(dev)
    qd, kd, vd = d(q), d(k.half()), d(VT)
    s0, s1 = d(torch.tensor(3000.0)), d(torch.tensor(9000.0))
    # a second request of the same shape with other queries: a merge that read a stale copy of a slot (the previous launch's partial
    # state, from a cache that should have been invalidated) reproduces request A's rows in request B
    q2d = d((torch.randn(B, H, L, 128) * 1.3).bfloat16())
    with _lib.tuning(attn_split=0):
        ref = ops.attention(qd, kd, vd).cpu()
        ref8 = ops.attention(qd, kd, vd, q_scale0=s0, q_scale1=s1, split=L // 3).cpu()
        ref_b = ops.attention(q2d, kd, vd).cpu()
    outs = []
    for _ in range(3):
        with _lib.tuning(attn_split=2):  # 2 = wherever a plan exists (the default, 1, takes it for thin last rounds only: rem <= 8 per XCD)
            outs.append((ops.attention(qd, kd, vd).cpu(), ops.attention(qd, kd, vd, q_scale0=s0, q_scale1=s1, split=L // 3).cpu(),
                         ops.attention(q2d, kd, vd).cpu()))
    got, got8, got_b = outs[0]
    for o, o8, ob in outs[1:]:
        assert torch.equal(o.view(torch.int16), got.view(torch.int16)) and torch.equal(o8.view(torch.uint8), got8.view(torch.uint8)) and \
            torch.equal(ob.view(torch.int16), got_b.view(torch.int16)), "balanced grid: launches differ"
    assert torch.isfinite(got).all() and torch.isfinite(got_b).all()
    vmax = v.abs().max().item()
    rel = lambda x, y: ((x.double() - y.double()).norm() / y.double().norm()).item()
    diff, diff_b = (got.float() - ref.float()).abs().max().item(), (got_b.float() - ref_b.float()).abs().max().item()
    same = (got == ref).float().mean().item()
    same8 = (got8.view(torch.uint8) == ref8.view(torch.uint8)).float().mean().item()
    print(f"B={B} H={H} L={L}: {len(plan['pieces'])} pieces per XCD after {plan['full_per_x']} whole tasks; balanced vs one workgroup per task: max |diff| {diff:.2e} "
          f"(second request {diff_b:.2e}), rel-L2 {rel(got, ref):.2e} / {rel(got_b, ref_b):.2e}, bf16 identical {same:.5f}, fp8 bytes identical {same8:.5f}")
    # a piece starts its own running max, so its P values are rounded to bf16 on another grid than the unsplit kernel's (what separates the
    # deferred from the exact-max build, which agree on ~0.8 of the outputs): a bf16 ulp on rows with few effective keys, nothing systematic
    assert max(diff, diff_b) <= 1e-2 * vmax and max(rel(got, ref), rel(got_b, ref_b)) <= 2.5e-3 and same8 >= 0.95
    # vs fp64 at every shape; H = 24: the first and the LAST head (the spiked one, a leftover task cut into pieces) keep the CPU time at seconds
    hs = list(range(H)) if H <= 8 else [0, H - 1]
    cut = lambda x: x.view(B, L, H, 128)[:, :, hs].reshape(B, L, len(hs) * 128)
    gate = ar.attention_gate(q[:, hs], k[:, hs], v[:, hs], True)
    ref64 = gate["ref"]
    st_s = ar.assert_attention_close(cut(got), q[:, hs], k[:, hs], v[:, hs], True, f"balanced_grid B={B} H={H} L={L} heads {hs[0]}..{hs[-1]} balanced", gate=gate)
    st_u = ar.assert_attention_close(cut(ref), q[:, hs], k[:, hs], v[:, hs], True, f"balanced_grid B={B} H={H} L={L} heads {hs[0]}..{hs[-1]} one workgroup per task", gate=gate)
    e_s, e_u = (cut(got).double() - ref64).abs().max().item(), (cut(ref).double() - ref64).abs().max().item()
    r_s, r_u = st_s["l2_got"], st_u["l2_got"]
    print(f"   vs fp64: balanced max |err| {e_s:.2e} rel-L2 {r_s:.3e}; one workgroup per task {e_u:.2e} / {r_u:.3e}")
    assert r_s <= 1.1 * r_u + 1e-5


@pytest.mark.parametrize("L,Lt", [(320, 64), (200, 40)])
def test_attention_rawq(ops, dev, L, Lt):
    """Raw-Q mode: QKNorm + RoPE applied to the query rows inside the attention kernel == qkv_rope's Q followed by attention
    (flux_model.py:158-176,60-65,41-45).  The row sum of squares is accumulated in a different order, so Q may differ by a rare
    bf16 ulp: compare the attention outputs (and against the oracle path)."""
    torch.manual_seed(9)
    B, H = 2, 3
    qkv = torch.randn(B, L, 3 * H * 128 + 64).bfloat16()
    s = [(1 + 0.1 * torch.randn(128)).bfloat16() for _ in range(4)]  # txt q,k ; img q,k
    img_ids = torch.zeros(B, L - Lt, 3, dtype=torch.bfloat16)
    img_ids[..., 1] = (torch.arange(L - Lt) // 8).bfloat16()
    img_ids[..., 2] = (torch.arange(L - Lt) % 8).bfloat16()
    ids = torch.cat((torch.zeros(B, Lt, 3, dtype=torch.bfloat16), img_ids), 1)
    pe6 = fo.rope_table(ids, [16, 56, 56], 10000, torch.bfloat16)
    pe = torch.stack((pe6[:, 0, :, :, 0, 0], pe6[:, 0, :, :, 1, 0]), -1).contiguous()
    d = lambda t: t.to(dev)
    qkv_d = d(qkv)[..., : 3 * H * 128]
    Q, K, VT = ops.qkv_rope(qkv_d, d(pe), d(s[0]), d(s[1]), d(s[2]), d(s[3]), split=Lt, heads=H)
    ref = ops.attention(Q, K, VT)
    Q2, K2, VT2 = ops.qkv_rope(qkv_d, d(pe), d(s[0]), d(s[1]), d(s[2]), d(s[3]), split=Lt, heads=H, skip_q=True)
    assert Q2 is None and torch.equal(K2, K) and torch.equal(VT2, VT)
    got = ops.attention_rawq(qkv_d, d(pe), d(s[0]), K2, VT2, qn_scale1=d(s[2]), split=Lt)
    torch.cuda.synchronize()
    diff = (got.float() - ref.float()).abs()
    vmax = qkv[..., 2 * H * 128 : 3 * H * 128].abs().max().item()
    assert diff.max().item() <= 1e-2 * vmax, f"raw-Q attention differs from two-kernel path: {diff.max().item()}"
    assert (got == ref).float().mean().item() >= 0.98
    # oracle: SDPA on the oracle's normalised + rotated q, k
    q, k, v = fo.split_heads(qkv[..., : 3 * H * 128], H)
    qn = torch.cat((fo.rms_norm(q[:, :, :Lt], s[0]), fo.rms_norm(q[:, :, Lt:], s[2])), 2)
    kn = torch.cat((fo.rms_norm(k[:, :, :Lt], s[1]), fo.rms_norm(k[:, :, Lt:], s[3])), 2)
    q_ref, k_ref = fo.apply_rope(qn, kn, pe6)
    gates = {f16: ar.attention_gate(q_ref, k_ref, v, f16) for f16 in (False, True)}
    o_ref = gates[False]["ref"]
    ar.assert_attention_close(got, q_ref, k_ref, v, False, f"rawq L={L} Lt={Lt} bf16 K", gate=gates[False])
    # folded kernel: fp16 K from the relayout kernel (exact copies of the bf16 values), Q scaled + fp16 on load
    _, K16, VT16 = ops.qkv_rope(qkv_d, d(pe), d(s[0]), d(s[1]), d(s[2]), d(s[3]), split=Lt, heads=H, skip_q=True, k_f16=True)
    assert K16.dtype == torch.float16 and torch.equal(K16.float(), K2.float()) and torch.equal(VT16, VT2)
    got16 = ops.attention_rawq(qkv_d, d(pe), d(s[0]), K16, VT16, qn_scale1=d(s[2]), split=Lt)
    e16, e0 = (got16.double().cpu() - o_ref).abs().max().item(), (got.double().cpu() - o_ref).abs().max().item()
    ar.assert_attention_close(got16, q_ref, k_ref, v, True, f"rawq L={L} Lt={Lt} fp16 K", gate=gates[True])
    r16 = ((got16.double().cpu() - o_ref).norm() / o_ref.norm()).item()
    r0 = ((got.double().cpu() - o_ref).norm() / o_ref.norm()).item()
    print(f"raw-Q attention vs fp64 on the oracle's q, k: bf16 K rel-L2 {r0:.3e} (max {e0:.2e}), fp16 K folded {r16:.3e} (max {e16:.2e})")
    assert r16 <= 1.15 * r0 + 1e-4


_EDGE_L = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 511, 513]
_F8_SCALES = {E5M2: (3000.0, 40000.0), E4M3: (200.0, 900.0)}  # the second of each saturates the largest outputs (clamp 57344 / 448)


def _edge_cases():
    """1 .. 9 key tiles (fewer than, exactly and more than the four the prologue prefetches), every residue of the ragged mask's two
    32-key halves around a tile edge, 1 .. 3 row blocks; two heads throughout, B x H = 2 x 3 on a subset, one long ragged sequence"""
    shapes = [(1, 2, L) for L in _EDGE_L] + [(2, 3, L) for L in (1, 33, 64, 129, 257, 513)] + [(1, 2, 3257)]
    return [(B, H, L, fam) for B, H, L in shapes for fam in ar.families_for(L)]


def _assert_f8_is_quantised_bf16(got8, out, split, fmt, what):
    """the fused fp8 output == float8_quantize.py:274-276 applied to the kernel's own bf16 output, rows < split with the first scale"""
    s0, s1 = (torch.tensor(s) for s in _F8_SCALES[fmt])
    want = torch.cat((fo.to_fp8_saturated(out[:, :split], s0, F8MAX[fmt]).to(F8T[fmt]), fo.to_fp8_saturated(out[:, split:], s1, F8MAX[fmt]).to(F8T[fmt])), 1)
    assert got8.dtype == F8T[fmt]
    ne = got8.float() != want.float()  # NaN (e4m3fn has one) compares unequal to itself: never accepted
    assert not ne.any(), f"{what}: {int(ne.sum())} fp8 outputs differ from quantise(own bf16 output)"


@pytest.mark.parametrize("B,H,L,family", _edge_cases())
def test_attention_edges(ops, dev, B, H, L, family):
    """K7 at the edges of its tiling against the per-element gate of tests/attention_ref.py (input families: attention_inputs there): both K
    formats (fp16 K = the folded kernel), deferred and exact running max; the fused fp8 output in BOTH formats and with the scale split
    inside, in front of and behind the rows == quantise(own bf16 output).                             flux_model.py:41-45"""
    from fluxmi import _lib

    q, k, v = ar.attention_inputs(family, B, H, L, seed=21)
    assert torch.equal(k.half().float(), k.float())
    d = lambda t: t.to(dev)
    qd, vd = d(q), d(_vt_layout(v, L))
    splits = sorted({0, L // 2, L})
    ref_A = ar.attention_ref64(q, k, v)
    for fold in (False, True):
        kd = d(k.half() if fold else k)
        for var in (0, 2):
            gate = ar.attention_gate(q, k, v, fold, exact=var == 2, ref_A=ref_A)  # exact max: one more rounding point (attention_model)
            what = f"edges B={B} H={H} L={L} {family} {'fp16' if fold else 'bf16'} K attn_var={var}"
            with _lib.tuning(attn_var=var, attn_abl=0):
                out = ops.attention(qd, kd, vd).cpu()
                got8 = {(fmt, sp): ops.attention(qd, kd, vd, q_scale0=d(torch.tensor(_F8_SCALES[fmt][0])), q_scale1=d(torch.tensor(_F8_SCALES[fmt][1])),
                                                 split=sp, fmt=fmt).cpu() for fmt in (E5M2, E4M3) for sp in splits}
            ar.assert_attention_close(out, q, k, v, fold, what, gate=gate)
            for (fmt, sp), g8 in got8.items():
                _assert_f8_is_quantised_bf16(g8, out, sp, fmt, f"{what} fmt={fmt} split={sp}")


@pytest.mark.parametrize("L", [33, 200])
def test_attention_padded_stride(ops, dev, L):
    """The ABI takes any Lp % 64 == 0, Lp >= L as the row stride of V^T (include/fluxmi.h): a wider stride must give the bits of the
    minimal one, and so must ANY finite content of the padding columns -- masked keys carry P = 0 exactly (exp2 of -1e30)."""
    B, H = 2, 2
    q, k, v = ar.attention_inputs("randn", B, H, L, seed=22)
    d = lambda t: t.to(dev)
    Lp0 = (L + 63) // 64 * 64
    s0, s1 = d(torch.tensor(3000.0)), d(torch.tensor(9000.0))
    g = torch.Generator().manual_seed(23)
    for fold in (False, True):
        kd = d(k.half() if fold else k)
        run = lambda vt: (ops.attention(d(q), kd, d(vt)).cpu(), ops.attention(d(q), kd, d(vt), q_scale0=s0, q_scale1=s1, split=L // 3).cpu())
        base, base8 = run(_vt_layout(v, L))
        ar.assert_attention_close(base, q, k, v, fold, f"padded_stride L={L} fold={fold} minimal Lp")
        for Lp in (Lp0, Lp0 + 64, Lp0 + 192):
            garbage = (torch.where(torch.rand(B, H, Lp, 128, generator=g) < 0.5, -1.0, 1.0) * 1e30).bfloat16()
            for fill in (None, garbage):
                if fill is None and Lp == Lp0:
                    continue  # the base itself
                out, out8 = run(_vt_layout(v, L, Lp=Lp, fill=fill))
                what = f"L={L} Lp={Lp} fold={fold} padding {'zero' if fill is None else 'garbage'}"
                assert torch.equal(out.view(torch.int16), base.view(torch.int16)), f"{what}: bf16 output differs from Lp={Lp0}"
                assert torch.equal(out8.view(torch.uint8), base8.view(torch.uint8)), f"{what}: fp8 output differs from Lp={Lp0}"


@pytest.mark.parametrize("L", [257, 33])
def test_attention_output_placement(ops, dev, L):
    """Output into a wider row at a column offset (how the single-stream block receives it: ld_out > H*128, col_off != 0), canary all
    around: every byte outside columns [col_off, col_off + H*128) of the B*L output rows keeps the canary, and so do Lp - L spare rows
    behind the last one (the rows of a batch are dense, sample b starts at row b*L, so a store for one of sample 0's clamped query rows
    >= L would land in sample 1's rows and break the equality below).  The inside == the plain call bit for bit.  fp8 at col_off = 8 is
    not 16-byte aligned: the 4-byte stores."""
    B, H = 2, 2
    q, k, v = ar.attention_inputs("randn", B, H, L, seed=24)
    d = lambda t: t.to(dev)
    qd, vd = d(q), d(_vt_layout(v, L))
    W, ld, spare = H * 128, H * 128 + 256, (L + 63) // 64 * 64 - L
    rows = B * L + spare
    for fold in (False, True):
        kd = d(k.half() if fold else k)
        plain = ops.attention(qd, kd, vd).cpu()
        ar.assert_attention_close(plain, q, k, v, fold, f"output_placement L={L} fold={fold}")
        for col in (0, 128):
            buf = torch.full((rows, ld), 0x5A5A, dtype=torch.int16, device=dev)
            ops.attention(qd, kd, vd, out=buf[: B * L].view(B, L, ld).view(torch.bfloat16), col_off=col)
            got = buf.cpu()
            assert torch.equal(got[: B * L, col : col + W], plain.view(torch.int16).reshape(B * L, W)), f"bf16 col_off={col} fold={fold}: inside differs"
            got[: B * L, col : col + W] = 0x5A5A
            assert (got == 0x5A5A).all(), f"bf16 col_off={col} fold={fold}: {int((got != 0x5A5A).sum())} elements written outside the output columns"
        for fmt in (E5M2, E4M3):
            s0, s1 = (d(torch.tensor(s)) for s in _F8_SCALES[fmt])
            plain8 = ops.attention(qd, kd, vd, q_scale0=s0, q_scale1=s1, split=L // 3, fmt=fmt).cpu()
            _assert_f8_is_quantised_bf16(plain8, plain, L // 3, fmt, f"output_placement L={L} fold={fold} fmt={fmt}")
            for col in (0, 128, 8):
                buf = torch.full((rows, ld), 0xA5, dtype=torch.uint8, device=dev)
                ops.attention(qd, kd, vd, q_scale0=s0, q_scale1=s1, split=L // 3, fmt=fmt, out=buf[: B * L].view(B, L, ld).view(F8T[fmt]), col_off=col)
                got = buf.cpu()
                assert torch.equal(got[: B * L, col : col + W], plain8.view(torch.uint8).reshape(B * L, W)), f"fp8 fmt={fmt} col_off={col} fold={fold}: inside differs"
                got[: B * L, col : col + W] = 0xA5
                assert (got == 0xA5).all(), f"fp8 fmt={fmt} col_off={col} fold={fold}: {int((got != 0xA5).sum())} bytes written outside the output columns"


@pytest.mark.parametrize("L,Lt", [(33, 8), (65, 1), (257, 64), (513, 0)])
def test_attention_rawq_edges(ops, dev, L, Lt):
    """Raw-Q mode (test_attention_rawq's construction) on ragged sequences, a one-row and an empty txt part, both K formats: against the
    oracle's normalised + rotated q, k through the per-element gate, and against qkv_rope + attention (the row sum of squares is
    accumulated in another order: a rare bf16 ulp in Q).                                   flux_model.py:158-176,60-65,41-45"""
    torch.manual_seed(91)
    B, H = 2, 3
    qkv = torch.randn(B, L, 3 * H * 128 + 64).bfloat16()
    s = [(1 + 0.1 * torch.randn(128)).bfloat16() for _ in range(4)]  # txt q,k ; img q,k
    img_ids = torch.zeros(B, L - Lt, 3, dtype=torch.bfloat16)
    img_ids[..., 1] = (torch.arange(L - Lt) // 8).bfloat16()
    img_ids[..., 2] = (torch.arange(L - Lt) % 8).bfloat16()
    ids = torch.cat((torch.zeros(B, Lt, 3, dtype=torch.bfloat16), img_ids), 1)
    pe6 = fo.rope_table(ids, [16, 56, 56], 10000, torch.bfloat16)
    pe = torch.stack((pe6[:, 0, :, :, 0, 0], pe6[:, 0, :, :, 1, 0]), -1).contiguous()
    q, k, v = fo.split_heads(qkv[..., : 3 * H * 128], H)
    qn = torch.cat((fo.rms_norm(q[:, :, :Lt], s[0]), fo.rms_norm(q[:, :, Lt:], s[2])), 2)
    kn = torch.cat((fo.rms_norm(k[:, :, :Lt], s[1]), fo.rms_norm(k[:, :, Lt:], s[3])), 2)
    q_ref, k_ref = fo.apply_rope(qn, kn, pe6)
    d = lambda t: t.to(dev)
    qkv_d = d(qkv)[..., : 3 * H * 128]
    for f16 in (False, True):
        Q, K, VT = ops.qkv_rope(qkv_d, d(pe), d(s[0]), d(s[1]), d(s[2]), d(s[3]), split=Lt, heads=H, k_f16=f16)
        assert K.dtype == (torch.float16 if f16 else torch.bfloat16)
        two = ops.attention(Q, K, VT).cpu()
        got = ops.attention_rawq(qkv_d, d(pe), d(s[0]), K, VT, qn_scale1=d(s[2]), split=Lt).cpu()
        what = f"rawq_edges L={L} Lt={Lt} {'fp16' if f16 else 'bf16'} K"
        ar.assert_attention_close(got, q_ref, k_ref, v, f16, what)
        same = (got == two).float().mean().item()
        assert same >= 0.98, f"{what}: raw-Q == qkv_rope + attention on {same:.4f} of the outputs"


@pytest.mark.parametrize("cfg", [13, 16])
def test_gemm_fused_kv_epilogue(ops, dev, cfg):
    """The qkv GEMM writing K (QKNorm + RoPE) and V^T (transposed, k-slot key order) straight from its epilogue
    (fluxmi_gemm_group_t.k_out / vt_out) == the plain GEMM followed by fluxmi_qkv_rope, two streams (txt rows, img rows)."""
    from fluxmi import _lib

    torch.manual_seed(12)
    Hh, Lt, Li, K = 2, 48, 272, 256     # heads, txt rows, img rows, in features
    HD, L = Hh * 128, Lt + Li
    Lp = (L + 63) // 64 * 64
    d = lambda t: t.to(dev)
    ws, bs, a8s = [], [], []
    sar = None
    for M, seed in ((Lt, 1), (Li, 2)):
        a8, w8, sar, sbr, bias = make_f8_problem(M, 3 * HD, K, E5M2, seed=seed)
        a8s.append(d(a8)); ws.append((d(w8), d(sbr))); bs.append(d(bias))
    sar = d(sar)
    s = [d((1 + 0.1 * torch.randn(128)).bfloat16()) for _ in range(4)]  # txt q,k ; img q,k
    ids = torch.zeros(1, L, 3, dtype=torch.bfloat16)
    ids[0, Lt:, 1] = (torch.arange(Li) // 16).bfloat16()
    ids[0, Lt:, 2] = (torch.arange(Li) % 16).bfloat16()
    pe6 = fo.rope_table(ids, [16, 56, 56], 10000, torch.bfloat16)
    pe = d(torch.stack((pe6[:, 0, :, :, 0, 0], pe6[:, 0, :, :, 1, 0]), -1).contiguous())
    # reference path: plain GEMM -> qkv buffer -> relayout kernel
    qkv = torch.zeros(1, L, 3 * HD, dtype=torch.bfloat16, device=dev)
    for st, (r0, M) in enumerate(((0, Lt), (Lt, Li))):
        ops.linear(a8s[st], ws[st][0], bs[st], sar, ws[st][1], out=qkv[0, r0 : r0 + M], tile_cfg=cfg)
    _, K_ref, VT_ref = ops.qkv_rope(qkv, pe, s[0], s[1], s[2], s[3], split=Lt, heads=Hh, skip_q=True)
    # fused path: one grouped launch, two groups
    qkv2 = torch.zeros_like(qkv)
    K_out = torch.zeros(1, Hh, L, 128, dtype=torch.bfloat16, device=dev)
    VT_out = torch.zeros(1, Hh, 128, Lp, dtype=torch.bfloat16, device=dev)
    groups = []
    for st, (r0, M) in enumerate(((0, Lt), (Lt, Li))):
        groups.append(ops.make_group(a8s[st].data_ptr(), ws[st][0].data_ptr(), bs[st].data_ptr(), sar.data_ptr(), ws[st][1].data_ptr(),
                                     qkv2[0, r0:].data_ptr(), M, K, 3 * HD, vt_out=VT_out.data_ptr(), vt_ld=Lp, tok0=r0,
                                     vt_rows=Lt if st == 0 else Lp - Lt, kv_col0=HD, heads=Hh, k_out=K_out.data_ptr(), pe=pe.data_ptr(),
                                     k_norm=s[1 if st == 0 else 3].data_ptr(), k_rows=L))
    ops.gemm_grouped(groups, 3 * HD, K, True, E5M2, _lib.EPI_BF16, cfg)
    torch.cuda.synchronize()
    assert torch.equal(qkv2[..., :HD], qkv[..., :HD])            # q columns still go to C
    assert torch.equal(VT_out, VT_ref)                            # V^T: same bf16 values, same layout, zero padded
    assert_bf16_close(K_out, K_ref, max_ulp=1, min_exact=0.999, what="fused K")  # row sums of squares in another order


def test_gemm_persistent_row_pair_weights(ops, dev):
    """fluxmi_gemm_group_t.W_pairs: the weight in the row-pair layout [N/2][K/64][2][64] (fluxmi_pair_rows) gives the persistent kernel full
    128-byte lines per K-step; same values -> every output byte equals the launch that reads W.  Two groups, ragged rows, the split epilogue
    (plain, table and V^T tiles), three tiles per workgroup; fluxmi_pair_rows against the same permutation in torch."""
    from fluxmi import _lib

    torch.manual_seed(5)
    Hh, K = 256, 768
    N = 3 * Hh + 1024
    Ms = [5000, 333]
    qs = torch.tensor(2.5, device=dev)
    lut = ops.build_quant_lut(qs, E5M2, act=1)
    one = torch.tensor(1.0, device=dev)
    ws = [(torch.randn(N, K, device=dev) * 0.5).to(torch.float8_e4m3fn) for _ in Ms]
    for w in ws:
        ref = w.view(torch.uint8).view(N // 2, 2, K // 64, 64).permute(0, 2, 1, 3).contiguous().view(N, K)
        assert torch.equal(ops.pair_rows(w).view(torch.uint8), ref)
    a8s = [(torch.randn(M, K, device=dev) * 2).to(torch.float8_e5m2) for M in Ms]
    bias = torch.randn(N, device=dev).bfloat16()

    def run(pairs):
        outs, groups, keep = [], [], []
        for M, a, w in zip(Ms, a8s, ws):
            Lp = (M + 63) // 64 * 64
            o = torch.full((M, 3 * Hh), float("nan"), dtype=torch.bfloat16, device=dev)
            o2 = torch.zeros(M, Hh + (N - 3 * Hh), dtype=torch.uint8, device=dev)
            vt = torch.zeros(Hh, Lp, dtype=torch.bfloat16, device=dev)
            kw = dict(C2=o2.data_ptr(), ldc2=o2.stride(0), split_n=3 * Hh, c2_col0=Hh, q_scale=qs.data_ptr(), q_lut=lut.data_ptr(),
                      vt_out=vt.data_ptr(), vt_ld=Lp, tok0=0, vt_rows=Lp, kv_col0=Hh, heads=Hh // 128)
            if pairs:
                wp = ops.pair_rows(w)
                keep.append(wp)
                kw.update(W_pairs=wp.data_ptr())
            outs += [o, o2, vt]
            groups.append(ops.make_group(a.data_ptr(), w.data_ptr(), bias.data_ptr(), one.data_ptr(), one.data_ptr(), o.data_ptr(), M, K, o.stride(0), **kw))
        ops.gemm_grouped(groups, N, K, True, E5M2, _lib.EPI_SPLIT, 18)
        torch.cuda.synchronize()
        return [x.view(torch.uint8) if x.dtype == torch.uint8 else x.view(torch.int16) for x in outs]

    for i, (x, y) in enumerate(zip(run(False), run(True))):
        assert torch.equal(x, y), f"output {i} differs with W_pairs"


@pytest.mark.parametrize("cfg", [16, 13])
def test_gemm_one_wave_kernel_row_pair_weights(ops, dev, cfg):
    """W_pairs through the one-wave-per-SIMD kernel (tile config 16: the step's mlp.2 / linear2 launches) and, since round 6, the ping-pong
    kernel (13: the proj launches): gate * y + x in place, ragged rows, two groups of which only ONE has a row-pair copy (a per-workgroup
    choice there); every byte equals the launch without copies."""
    from fluxmi import _lib

    torch.manual_seed(6)
    N, K, Ms = 768, 2048, [700, 300]
    one = torch.tensor(1.0, device=dev)
    ws = [(torch.randn(N, K, device=dev) * 0.5).to(torch.float8_e4m3fn) for _ in Ms]
    a8s = [(torch.randn(M, K, device=dev) * 2).to(torch.float8_e5m2) for M in Ms]
    gate = torch.randn(N, device=dev).bfloat16()
    x0 = [torch.randn(M, N, device=dev).bfloat16() for M in Ms]

    def run(pairs):
        outs, groups, keep = [], [], []
        for gi, (M, a, w) in enumerate(zip(Ms, a8s, ws)):
            o = x0[gi].clone()
            kw = dict(gate=gate.data_ptr(), resid=o.data_ptr(), ldr=N)
            if pairs and gi == 0:
                wp = ops.pair_rows(w)
                keep.append(wp)
                kw.update(W_pairs=wp.data_ptr())
            outs.append(o)
            groups.append(ops.make_group(a.data_ptr(), w.data_ptr(), None, one.data_ptr(), one.data_ptr(), o.data_ptr(), M, K, N, **kw))
        ops.gemm_grouped(groups, N, K, True, E5M2, _lib.EPI_GATE_RESID, cfg)
        torch.cuda.synchronize()
        return outs

    for x, y in zip(run(False), run(True)):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))


@pytest.mark.parametrize("cfg", [13, 16, 17, 113 + 4])
def test_gemm_bf16_row_pair_weights(ops, dev, cfg):
    """Round 6: W_pairs for BF16 weights (row bytes K * 2): the bf16 flow's 64-byte-K-step kernels -- ping-pong (13), one-wave-per-SIMD (16 / 17) and the
    split-K build of 13 -- read the row-pair copy and give the bits of the plain launch (Flux-schnell's M = 512 launches stream 24 - 132 MB of weights
    each: half lines cost them as they cost the fp8 step).                                  flux_model.py:154-155 (nn.Linear), layout only"""
    from fluxmi import _lib

    torch.manual_seed(8)
    M, N, K = 512, 3072, 6144
    a = torch.randn(M, K, device=dev).bfloat16()
    w = (torch.randn(N, K, device=dev) * 0.02).bfloat16()
    wp = ops.pair_rows(w)
    bias = torch.randn(N, device=dev).bfloat16()
    gate = torch.randn(N, device=dev).bfloat16()
    for epi in (_lib.EPI_BF16, _lib.EPI_GATE_RESID):
        outs = []
        for pairs in (False, True):
            o = torch.randn(M, N, device=dev, generator=torch.Generator(device=dev).manual_seed(3)).bfloat16()
            kw = dict(gate=gate.data_ptr(), resid=o.data_ptr(), ldr=N) if epi == _lib.EPI_GATE_RESID else {}
            g = ops.make_group(a.data_ptr(), w.data_ptr(), bias.data_ptr(), None, None, o.data_ptr(), M, K, N, W_pairs=wp.data_ptr() if pairs else None, **kw)
            ops.gemm_grouped([g], N, K, False, E5M2, epi, cfg)
            torch.cuda.synchronize()
            outs.append(o.view(torch.int16).clone())
        assert torch.equal(outs[0], outs[1]), f"tile config {cfg}, epilogue {epi}: bf16 W_pairs changes the result"


@pytest.mark.parametrize("k_f16", [False, True])
@pytest.mark.parametrize("epi", ["bf16", "split"])
def test_gemm_persistent_fused_k(ops, dev, k_f16, epi):
    """The persistent kernel's fused-K tiles (QKNorm on the accumulators, sums of squares swapped between the two waves of a head, RoPE
    after the transposition: csrc/gemm_persist.hip) == the plain GEMM followed by fluxmi_qkv_rope, BIT FOR BIT (the sums run in the
    relayout kernel's order), bf16 and fp16 K; two streams with their own key scales, a ragged last tile per stream, three tiles per
    workgroup, q columns still in C, V^T from the same launch; `split`: the single-block linear1 form (table tiles in the same launch).
    flux_model.py:158-176,60-65,351-354"""
    from fluxmi import _lib

    torch.manual_seed(31)
    Hh, K = 2, 512
    HD = Hh * 128
    Lt, Li = 304, 21777 if epi == "bf16" else 9000   # bf16: 2 + 86 row tiles x 3 column tiles = 264 tiles on 256 workgroups
    L = Lt + Li
    Lp = (L + 63) // 64 * 64
    N = 3 * HD + (1024 if epi == "split" else 0)
    streams = ((0, Lt), (Lt, Li))
    ws, a8s, bs = [], [], []
    for r0, M in streams:
        a8s.append((torch.randn(M, K, device=dev) * 2).to(torch.float8_e5m2))
        ws.append((torch.randn(N, K, device=dev) * 0.5).to(torch.float8_e4m3fn))
        bs.append(torch.randn(N, device=dev).bfloat16())
    sar, sbr = torch.tensor(0.41, device=dev), torch.tensor(0.77, device=dev)
    s = [(1 + 0.1 * torch.randn(128, device=dev)).bfloat16() for _ in range(4)]  # txt q,k ; img q,k
    ids = torch.zeros(1, L, 3, dtype=torch.bfloat16)
    ids[0, Lt:, 1] = (torch.arange(Li) // 150).bfloat16()
    ids[0, Lt:, 2] = (torch.arange(Li) % 150).bfloat16()
    pe6 = fo.rope_table(ids, [16, 56, 56], 10000, torch.bfloat16)
    pe = torch.stack((pe6[:, 0, :, :, 0, 0], pe6[:, 0, :, :, 1, 0]), -1).contiguous().to(dev)
    qs = torch.tensor(3.0, device=dev)
    lut = ops.build_quant_lut(qs, E5M2, act=1)
    e = _lib.EPI_BF16 if epi == "bf16" else _lib.EPI_SPLIT

    def run(cfg, fused_k):
        qkv = torch.full((1, L, 3 * HD), float("nan"), dtype=torch.bfloat16, device=dev)
        c2 = torch.zeros(L, HD + (N - 3 * HD), dtype=torch.uint8, device=dev)
        K_out = torch.zeros(1, Hh, L, 128, dtype=torch.float16 if k_f16 else torch.bfloat16, device=dev)
        VT_out = torch.zeros(1, Hh, 128, Lp, dtype=torch.bfloat16, device=dev)
        groups = []
        for st, (r0, M) in enumerate(streams):
            kw = dict(vt_out=VT_out.data_ptr(), vt_ld=Lp, tok0=r0, vt_rows=Lt if st == 0 else Lp - Lt, kv_col0=HD, heads=Hh)
            if fused_k:
                kw.update(k_out=K_out.data_ptr(), pe=pe.data_ptr(), k_norm=s[1 if st == 0 else 3].data_ptr(), k_rows=L, k_f16=k_f16)
            if epi == "split":
                kw.update(C2=c2[r0:].data_ptr(), ldc2=c2.stride(0), split_n=3 * HD, c2_col0=HD, q_scale=qs.data_ptr(), q_lut=lut.data_ptr())
            groups.append(ops.make_group(a8s[st].data_ptr(), ws[st].data_ptr(), bs[st].data_ptr(), sar.data_ptr(), sbr.data_ptr(),
                                         qkv[0, r0:].data_ptr(), M, K, 3 * HD, **kw))
        ops.gemm_grouped(groups, N, K, True, E5M2, e, cfg)
        torch.cuda.synchronize()
        return qkv, K_out, VT_out, c2

    qkv, _, VT_ref, c2_ref = run(13, False)
    _, K_ref, _ = ops.qkv_rope(torch.nan_to_num(qkv), pe, s[0], s[1], s[2], s[3], split=Lt, heads=Hh, skip_q=True, k_f16=k_f16)
    qkv2, K_out, VT_out, c2 = run(18, True)
    assert torch.equal(qkv2[..., :HD], qkv[..., :HD])              # q columns still go to C
    assert torch.isnan(qkv2[..., HD : 2 * HD].float()).all()        # the K columns do not
    assert torch.equal(VT_out, VT_ref)
    assert torch.equal(c2, c2_ref)
    same = (K_out.view(torch.int16) == K_ref.view(torch.int16)).float().mean().item()
    assert same == 1.0, f"fused K differs from the relayout kernel's on {1 - same:.3e} of the elements"
    # the one-tile-per-workgroup kernels' fused K adds the squares in another order: 1 / rms may differ in its last bit, i.e. an element by
    # one bf16 ulp of the rotation's operands (more "ulps" where the rotation cancels) -- almost all elements identical, none far off
    _, K13, _, _ = run(13, True)
    d = (K13.float() - K_ref.float()).abs()
    assert (K13 == K_ref).float().mean().item() >= 0.999 and d.max().item() <= 2.0 ** -6 * K_ref.float().abs().max().item()

@pytest.mark.parametrize("K", [256, 320, 512, 3072])
def test_quant_lut_epilogue(ops, dev, K):
    """Table-driven GELU + quantise epilogue (fluxmi_gemm_group_t.q_lut) == the computed one, bit for bit, for GELU_QUANT and for the
    mlp columns of SPLIT; the table itself == the oracle's chain over all 65536 bf16 patterns.  Several K (ring phases at the
    end of the main loop differ: 4, 5, 8, 48 K-steps)."""
    from fluxmi import _lib

    M, N = 384, 1024
    a8, w8, sar, sbr, bias = make_f8_problem(M, N, K, E5M2, seed=21)
    d = lambda t: t.to(dev)
    qs = torch.tensor(41.0, dtype=torch.float32)
    lut = ops.build_quant_lut(d(qs), E5M2, act=1)
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    ref_lut = fo.to_fp8_saturated(F.gelu(bits, approximate="tanh"), qs, 57344.0).to(torch.float8_e5m2).view(torch.uint8)
    same = lut.cpu() == ref_lut
    nan = torch.isnan(bits.float())
    assert same[~nan].float().mean().item() >= 0.999  # (rare 1-ulp GELU flips, as in test_gelu_table)
    args = (d(a8), d(w8), d(bias), d(sar), d(sbr))
    ref = ops.linear(*args, epilogue=_lib.EPI_GELU_QUANT, q_scale=d(qs), tile_cfg=13)
    got = ops.linear(*args, epilogue=_lib.EPI_GELU_QUANT, q_scale=d(qs), tile_cfg=13, q_lut=lut)
    assert torch.equal(got.view(torch.uint8), ref.view(torch.uint8))
    # split: first 512 columns plain bf16, the rest GELU + quantise into a wider buffer at a column offset
    split = 512
    o1, o2 = (torch.zeros(M, split, dtype=torch.bfloat16, device=dev) for _ in range(2))
    w1_, w2_ = (torch.zeros(M, 128 + N - split, dtype=torch.float8_e5m2, device=dev) for _ in range(2))
    ops.linear(*args, epilogue=_lib.EPI_SPLIT, q_scale=d(qs), out=o1, out2=w1_, split_n=split, c2_col0=128, tile_cfg=13)
    ops.linear(*args, epilogue=_lib.EPI_SPLIT, q_scale=d(qs), out=o2, out2=w2_, split_n=split, c2_col0=128, tile_cfg=13, q_lut=lut)
    assert torch.equal(o1, o2) and torch.equal(w1_.view(torch.uint8), w2_.view(torch.uint8))


@pytest.mark.parametrize("B,Hi,Wi,C,Cout,up", [(1, 24, 40, 128, 128, 1), (2, 16, 24, 256, 128, 2), (1, 32, 32, 128, 256, -2), (1, 64, 64, 512, 512, 1),
                                               (1, 9, 13, 64, 128, 1), (1, 5, 7, 128, 128, 2)])
def test_conv3x3_implicit_equals_im2col_gemm(ops, dev, B, Hi, Wi, C, Cout, up):
    """fluxmi_conv3x3 (round 6): the 3x3 convolution as an IMPLICIT GEMM -- the 128 x 128 tile kernel gathers every 128-byte K-step (64 channels of
    one tap) from the NHWC input in its LDS-DMA address computation, out-of-image taps through a zero page -- must equal the GEMM on
    fluxmi_im2col3x3's explicit patch matrix BIT FOR BIT (same K order, same MFMAs, same tile config): stride 1 / pad 1, the folded 2x nearest
    upsample, the stride-2 right/bottom-padded window; odd sizes (ragged last tile), two images, plain and residual epilogues; and it matches
    torch's conv2d to bf16 accuracy.                                          reference modules/autoencoder.py:55-120 (Conv2d 3x3)"""
    from fluxmi import _lib

    torch.manual_seed(17)
    if up == -2:
        Hi, Wi = Hi * 2, Wi * 2
    x = torch.randn(B, Hi, Wi, C, device=dev).bfloat16()
    w = (torch.randn(Cout, C, 3, 3, device=dev) * (9 * C) ** -0.5).bfloat16()
    w2 = w.permute(0, 2, 3, 1).reshape(Cout, 9 * C).contiguous()  # [Cout][dy][dx][C]
    bias = torch.randn(Cout, device=dev).bfloat16()
    col = ops.im2col3x3(x, up)
    ref = torch.empty(col.shape[0], Cout, dtype=torch.bfloat16, device=dev)
    ops.linear(col, w2, bias, out=ref, tile_cfg=2)
    got = ops.conv3x3(x, w2, bias, up)
    H, W = got.shape[1], got.shape[2]
    assert got.shape == (B, H, W, Cout) and ref.shape[0] == B * H * W
    assert torch.equal(got.view(-1, Cout).view(torch.int16), ref.view(torch.int16)), \
        f"implicit conv differs from im2col + GEMM: {(got.view(-1, Cout) != ref).float().mean().item():.2e} of the elements"
    # residual epilogue: out = resid + 1 * y
    resid = torch.randn(B, H, W, Cout, device=dev).bfloat16()
    ones = torch.ones(Cout, dtype=torch.bfloat16, device=dev)
    ref_r = torch.empty_like(ref)
    ops.linear(col, w2, bias, epilogue=_lib.EPI_GATE_RESID, gate=ones, resid=resid.view(-1, Cout), out=ref_r, tile_cfg=2)
    got_r = ops.conv3x3(x, w2, bias, up, resid=resid)
    assert torch.equal(got_r.view(-1, Cout).view(torch.int16), ref_r.view(torch.int16))
    # against torch (fp32 conv of the bf16 values), bf16 accuracy
    xin = x.float().permute(0, 3, 1, 2)
    if up == 2:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    if up == -2:
        t = F.conv2d(F.pad(xin, (0, 1, 0, 1)), w.float(), bias.float(), stride=2)
    else:
        t = F.conv2d(xin, w.float(), bias.float(), padding=1)
    t = t.permute(0, 2, 3, 1)
    err = (got.float() - t).abs().max().item()
    assert err <= 2.0 ** -6 * max(1.0, t.abs().max().item()), f"implicit conv vs torch conv2d: max |err| {err:.3e}"


def test_lora_fuse(ops, dev):
    """Config 5: dequant + B@A + requant on device (lora_loading.py:509-577,615-631 -> float8_quantize.py:209-212)."""
    torch.manual_seed(12)
    N, K, R = 384, 256, 16
    w = (torch.randn(N, K) * 0.05).bfloat16()
    for chunks in (1, 3, 4):  # 1 = plain, 3 = fused qkv ("uneven rank"), 4 = single-block linear1 from a diffusers-format file (q|k|v|mlp)
        st = fo.F8LinearState(w, None)
        A = torch.randn(chunks * R, K) * 0.1
        Bm = torch.randn(N, R) * 0.1
        alpha = 8.0
        delta = fo.lora_delta(A, Bm, alpha, 0.8)
        st_ref_w = (st.dequantized_weight() + delta).type(torch.bfloat16)
        st2 = fo.F8LinearState(w, None)
        q = st2.float8_data.to(dev).clone()
        sc, rc = st2.scale.to(dev).clone(), st2.scale_reciprocal.to(dev).clone()
        A_scaled = (A * alpha / R)
        ops.lora_fuse_f8(q, sc, rc, Bm.to(dev), A_scaled.to(dev), 0.8, n_chunks=chunks)
        st.set_weight_tensor(st_ref_w)
        assert abs(sc.item() - st.scale.item()) <= 1e-6 * st.scale.item()
        assert_f8_close(q, st.float8_data, max_ulp=1, min_exact=0.995, what=f"lora fuse chunks={chunks}")


# ---- VAE decoder pieces -----------------------------------------------------------------------------
@pytest.mark.parametrize("up", [1, 2, -2])
def test_im2col3x3(ops, dev, up):
    """Patch matrix == F.unfold of the (nearest-upsampled / right-bottom-padded, stride 2) NCHW image, columns reordered (dy, dx, c)."""
    torch.manual_seed(31)
    B, Hi, Wi, C = 2, 6, 10, 16
    x = torch.randn(B, Hi, Wi, C).bfloat16()
    col = ops.im2col3x3(x.to(dev), up).cpu()
    xn = x.permute(0, 3, 1, 2).float()
    if up == 2:
        xn = F.interpolate(xn, scale_factor=2.0, mode="nearest")
    if up == -2:  # Downsample.forward, reference modules/autoencoder.py:103-107
        H, W = Hi // 2, Wi // 2
        ref = F.unfold(F.pad(xn, (0, 1, 0, 1)), kernel_size=3, stride=2).view(B, C, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 9 * C)
        assert torch.equal(col.float(), ref)
        return
    H, W = Hi * up, Wi * up
    ref = F.unfold(xn, kernel_size=3, padding=1).view(B, C, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 9 * C)
    assert torch.equal(col.float(), ref)


@pytest.mark.parametrize("C,swish", [(32, True), (64, False), (512, True)])
def test_groupnorm(ops, dev, C, swish):
    torch.manual_seed(32)
    B, P = 2, 5000
    x = (torch.randn(B, P, C) * 2 + 0.5).bfloat16()
    ga, be = (1 + 0.1 * torch.randn(C)).bfloat16(), (0.1 * torch.randn(C)).bfloat16()
    ref = F.group_norm(x.float().permute(0, 2, 1), 32, ga.float(), be.float(), eps=1e-6)
    if swish:
        ref = ref * torch.sigmoid(ref)
    ref = ref.permute(0, 2, 1).bfloat16()
    got = ops.groupnorm(x.to(dev), ga.to(dev), be.to(dev), swish=swish).cpu()
    # values near zero come out of a cancellation ((x - mean) * rstd * gamma + beta): 1 bf16 ulp at the magnitude of the operands
    assert_close_mag(got, ref, mag=0.25, ulps=1, min_exact=0.99, what="groupnorm")


def test_softmax_rows(ops, dev):
    torch.manual_seed(33)
    S = (torch.randn(300, 1024) * 6).bfloat16()
    ref = torch.softmax(S.float() * 0.125, dim=-1).bfloat16()
    got = ops.softmax_rows(S.to(dev), 0.125).cpu()
    assert_bf16_close(got, ref, max_ulp=1, min_exact=0.99, what="softmax rows")


# ---- text-conditioning encoder pieces -----------------------------------------------------------------
@pytest.mark.parametrize("D,rms", [(64, True), (4096, True), (768, False), (128, False)])
def test_row_norm(ops, dev, D, rms):
    """T5LayerNorm (fp32 variance, bf16 rounding before the weight) / LayerNorm with the rounding points of the HF modules in bf16."""
    torch.manual_seed(41)
    x = (torch.randn(37, D) * 3 + (0.0 if rms else 1.5)).bfloat16()
    w = (1 + 0.2 * torch.randn(D)).bfloat16()
    b = (0.1 * torch.randn(D)).bfloat16()
    if rms:
        h = (x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-6)).bfloat16()
        ref = w * h
    else:
        ref = F.layer_norm(x.float(), (D,), w.float(), b.float(), 1e-5).bfloat16()
    got = ops.row_norm(x.to(dev), w.to(dev), None if rms else b.to(dev), eps=1e-6 if rms else 1e-5, rms=rms).cpu()
    assert_bf16_close(got, ref, max_ulp=1, min_exact=0.98, what=f"row_norm D={D} rms={rms}")


def test_act_mul(ops, dev):
    torch.manual_seed(42)
    x = (torch.randn(50, 512) * 2).bfloat16()
    a, b = x[:, :256].float(), x[:, 256:].float()
    gelu = (0.5 * a * (1.0 + torch.tanh(0.7978845608028654 * (a + 0.044715 * a ** 3)))).bfloat16()
    assert_bf16_close(ops.act_mul(x.to(dev), gated=True).cpu(), (gelu.float() * b).bfloat16(), max_ulp=1, min_exact=0.97, what="gated gelu_new")
    q = (x.float() * torch.sigmoid(1.702 * x.float())).bfloat16()
    assert_bf16_close(ops.act_mul(x.to(dev), gated=False).cpu(), q, max_ulp=1, min_exact=0.98, what="quick_gelu")


@pytest.mark.parametrize("L,H,causal", [(40, 3, False), (512, 4, False), (77, 2, True), (32, 1, True)])
def test_text_attention(ops, dev, L, H, causal):
    """head_dim-64 attention of the text encoders vs fp32 math on the same bf16 inputs: T5 style (no scaling, additive
    relative-position bias as a function of key - query, no mask) and CLIP style (1/sqrt(d), causal mask, v bias added after P V)."""
    torch.manual_seed(43)
    Lp = (L + 31) // 32 * 32
    qk = torch.zeros(Lp, 2 * H * 64)
    qk[:L] = torch.randn(L, 2 * H * 64) * (0.35 if not causal else 1.0)
    qk = qk.bfloat16()
    v = torch.zeros(Lp, H * 64)
    v[:L] = torch.randn(L, H * 64)
    v = v.bfloat16()
    vb = (0.3 * torch.randn(H * 64)).bfloat16() if causal else None
    rel = None if causal else torch.randn(H, 2 * Lp)
    scale = 0.125 if causal else 1.0
    q, k = qk[:, : H * 64], qk[:, H * 64:]
    qh, kh, vh = (t[:L].float().view(L, H, 64).transpose(0, 1) for t in (q, k, v))
    s = torch.matmul(qh, kh.transpose(-1, -2)) * scale
    if rel is not None:
        pos = torch.arange(L)
        s = s + rel[:, (pos[None, :] - pos[:, None]) + Lp]
    if causal:
        s = s + torch.full((L, L), float("-inf")).triu(1)
    p = torch.softmax(s, -1).bfloat16().float()
    o = torch.matmul(p, vh)
    if vb is not None:
        o = o.bfloat16().float() + vb.float().view(H, 1, 64)
    ref = o.transpose(0, 1).reshape(L, H * 64)
    d = lambda t: t.to(dev)
    qkd = d(qk)
    got = ops.text_attention(qkd[:, : H * 64], qkd[:, H * 64:], d(v.t().contiguous()), L, H, scale=scale, causal=causal,
                             rel_bias=d(rel) if rel is not None else None, v_bias=d(vb) if vb is not None else None).cpu()
    assert torch.all(got[L:] == 0)
    err = (got[:L].float() - ref).abs()
    tol = 2.0 ** -8 * ref.abs().clamp(min=0.05) + 4e-3  # one bf16 ulp of the output + the bf16 rounding of P (<= 2^-9 relative per term)
    assert bool((err <= tol).all()), f"text attention L={L} H={H} causal={causal}: max err {err.max():.3e} (ref max {ref.abs().max():.2f})"
