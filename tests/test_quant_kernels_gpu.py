"""The fp8 quantise family of csrc/elementwise.hip -- quantize_act, amax, quantize_weight, dequant, build_quant_lut(act=0) and the LoRA re-fuse
chain of fluxmi_lora_fuse_f8 -- against the CPU oracle chain restated in tests/quant_refs.py: strided views with poisoned gaps, the second
trip of every grid-stride loop, non-finite inputs, every fp8 byte, ragged K and ranks 1 to 128.

The gate is equality of bits everywhere but the random-adapter fuse, whose gate knows the elements an fp32 summation order may move
(quant_refs.gate_fuse_random).  tests/test_quant_refs_cpu.py shows that every case here rejects the wrong kernels it is built for.  Every test
prints its count of mismatching bytes before it asserts.
"""
import pytest
import torch

import quant_refs as qr
from quant_refs import E4M3, F8T, FMT_NAME, FMTS, byte_mismatch, f32_bits, f32_mismatch, scalar, u8

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(dev):
    from fluxmi import ops as _ops

    return _ops


def fmt_id(v):
    return FMT_NAME.get(v, str(v)) if isinstance(v, int) else str(v).replace(" ", "")


def same_scalar(got, exp):
    return f32_bits(got.cpu()).item() == f32_bits(exp).item()


# ---- 1. quantize_act -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", qr.QUANT_STRIDE_CASES, ids=fmt_id)
def test_quantize_act_strided_views(ops, dev, case, fmt):
    """input and output are column slices of wider buffers (ld_in != ld_out); the input gap holds NaN and 3e38, the output gap and the two
    guard rows a sentinel byte that must survive"""
    cols, rows, ld_in, ld_out, c0_in, c0_out = case
    xbuf = qr.quant_stride_inputs(cols, rows, ld_in, c0_in, fmt)
    scale = qr.quant_stride_scale(fmt)
    exp = qr.quant_stride_expected(xbuf, cols, rows, ld_in, ld_out, c0_in, c0_out, scale, fmt)
    xd = xbuf.to(dev)
    obuf = torch.full((rows + qr.GUARD_ROWS, ld_out), qr.OUT_SENTINEL, dtype=torch.uint8, device=dev).view(F8T[fmt])
    ops.quantize_act(xd[:rows, c0_in:c0_in + cols], scale.to(dev), fmt, out=obuf[:rows, c0_out:c0_out + cols])
    bad = byte_mismatch(obuf, exp, fmt)
    print(f"quantize_act {FMT_NAME[fmt]} cols={cols} ld {ld_in}->{ld_out}: {int(bad.sum())} mismatching bytes of {bad.numel()} (gap included)")
    assert not bool(bad.any()), f"first mismatches at {bad.nonzero()[:5].tolist()}"


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
def test_quantize_act_second_trip(ops, dev, fmt):
    """1026 x 8200 = 1,051,650 vectors: the grid-stride loop takes a second trip over the last 3074, which carry values of their own"""
    x = qr.quant_trip2_input()
    scale = qr.quant_stride_scale(fmt)
    exp = qr.quant_trip2_expected(x, scale, fmt)
    out = torch.full(x.shape, qr.OUT_SENTINEL, dtype=torch.uint8, device=dev).view(F8T[fmt])
    ops.quantize_act(x.to(dev), scale.to(dev), fmt, out=out)
    bad = byte_mismatch(out, exp, fmt)
    print(f"quantize_act {FMT_NAME[fmt]} second trip: {int(bad.sum())} mismatching bytes of {bad.numel()}, {int(bad[-3:].sum())} in the last three rows")
    assert not bool(bad.any()), f"first mismatches at {bad.nonzero()[:5].tolist()}"


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
def test_quantize_act_all_patterns_with_specials(ops, dev, fmt):
    """all 65536 bf16 patterns -- +-inf, every NaN, -0, the subnormals, values whose product with the scale overflows bf16 -- at every scale:
    +-inf give +-max, NaN gives a NaN byte and never a finite one, the rest follow the oracle bit for bit"""
    x = qr.all_bf16_patterns().view(-1, 8)
    xd = x.to(dev)
    for s in qr.quant_scales(fmt):
        exp = qr.quantize_ref(x, scalar(s), fmt)
        got = ops.quantize_act(xd, scalar(s).to(dev), fmt)
        bad = byte_mismatch(got, exp, fmt)
        nan_in = torch.isnan(x)
        finite_from_nan = int((nan_in & ~qr.f8_is_nan(got.cpu(), fmt)).sum())
        print(f"quantize_act {FMT_NAME[fmt]} scale={s:g}: {int(bad.sum())} mismatching bytes of 65536, {finite_from_nan} NaN inputs became finite")
        assert finite_from_nan == 0
        assert not bool(bad.any()), f"scale {s}: first inputs {x[bad][:5].float().tolist()}"
        inf = torch.isinf(x)
        assert torch.equal(u8(got.cpu())[inf], u8((torch.sign(x[inf].float()) * qr.F8MAX[fmt]).to(F8T[fmt])))


# ---- 2. amax ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", qr.AMAX_CASES)
def test_amax(ops, dev, name):
    """== x.abs().max().float() wherever no NaN is involved; a NaN element is skipped (the contract in include/fluxmi.h); the gap of a
    strided view holds 3e38 and is never read; *amax = max(*amax, ...)"""
    xbuf, rows, cols, c0, preset, _, nan_free = qr.amax_case(name)
    exp = qr.amax_ref(xbuf, rows, cols, c0, preset)
    if nan_free:
        assert same_scalar(exp, torch.maximum(scalar(preset), qr.amax_oracle(xbuf, rows, cols, c0)))
    out = scalar(preset).to(dev)
    got = ops.amax(xbuf.to(dev)[:rows, c0:c0 + cols], out=out)
    print(f"amax {name}: got {got.item()!r}, expected {exp.item()!r}")
    assert same_scalar(got, exp)


# ---- 3. quantize_weight ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("shape", qr.QW_SHAPES, ids=fmt_id)
def test_quantize_weight(ops, dev, shape, fmt):
    """(q, scale, recip) bit-exact vs fo.quantize_weight at every amplitude and every place of the dominant element, and for an all-zero weight"""
    N, K = shape
    total = 0
    for amp in qr.QW_AMPS:
        for where, pos in qr.qw_positions(N, K).items():
            w = qr.qw_weight(N, K, amp, pos)
            q_ref, s_ref, r_ref = qr.quantize_weight_ref(w, fmt)
            q, s, r = ops.quantize_weight(w.to(dev), fmt)
            bad = byte_mismatch(q, q_ref, fmt)
            total += int(bad.sum())
            print(f"quantize_weight {FMT_NAME[fmt]} {N}x{K} amp={amp:g} dominant {where}: {int(bad.sum())} mismatching bytes, scale {s.item()!r} vs {s_ref.item()!r}")
            assert same_scalar(s, s_ref) and same_scalar(r, r_ref), f"amp {amp} {where}: scale {s.item()!r} vs {s_ref.item()!r}, recip {r.item()!r} vs {r_ref.item()!r}"
            assert not bool(bad.any()), f"amp {amp} {where}: first mismatches at {bad.nonzero()[:5].tolist()}"
    w0 = torch.zeros(N, K).bfloat16()
    q_ref, s_ref, r_ref = qr.quantize_weight_ref(w0, fmt)
    q, s, r = ops.quantize_weight(w0.to(dev), fmt)
    assert s_ref.item() == qr.F8MAX[fmt] and same_scalar(s, s_ref) and same_scalar(r, r_ref)
    assert not bool(byte_mismatch(q, q_ref, fmt).any())
    assert total == 0


# ---- 4. dequant ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("n", [256, qr.DEQ_BIG_N])
def test_dequant(ops, dev, n, fmt):
    """every byte at every reciprocal, bit-exact vs q.float().mul(recip); NaN bytes give NaN, e5m2's inf bytes follow the reference; the large
    n takes a second trip of the grid-stride loop"""
    qb = qr.dequant_bytes(n)
    qd = qb.view(F8T[fmt]).to(dev)
    for recip in qr.DEQ_RECIPS:
        exp = qr.dequant_ref(qb, scalar(recip), fmt)
        got = ops.dequant(qd, scalar(recip).to(dev)).cpu()
        bad = f32_mismatch(got, exp)
        print(f"dequant {FMT_NAME[fmt]} n={n} recip={recip:g}: {int(bad.sum())} mismatching values, {int(bad[qr.FLAT_TRIP:].sum())} in the second trip")
        assert not bool(bad.any()), f"recip {recip}: first mismatches at {bad.nonzero()[:5].flatten().tolist()}, bytes {qb[bad][:5].tolist()}"


# ---- 5. lora_fuse_f8, exact-arithmetic adapters ----------------------------------------------------------------------------------------
def run_fuse(ops, dev, st, Bm, A, ls, chunks):
    """in place on clones of the weight and its scalars -> (q, scale, recip) on the device"""
    q = st.float8_data.to(dev).clone()
    sc, rc = st.scale.to(dev).clone(), st.scale_reciprocal.to(dev).clone()
    ops.lora_fuse_f8(q, sc, rc, Bm.to(dev), A.to(dev), ls, n_chunks=chunks)
    return q, sc, rc


@pytest.mark.parametrize("case", qr.FUSE_EXACT_CASES, ids=fmt_id)
def test_lora_fuse_exact_adapters(ops, dev, case):
    """integer-valued adapters make the delta exact in fp32 in any order: q bytes, scale and recip equal the oracle chain bit for bit.  K = 264
    and 8072 run the ragged last workgroup of the delta kernel, (520, 8072) the second trip of dequant, axpy_f32 and quantize_f32."""
    N, K, R, chunks = case
    st, Bm, A = qr.fuse_exact_inputs(N, K, R, chunks)
    total = 0
    for ls in qr.FUSE_SCALES:
        q_ref, s_ref, r_ref = qr.fuse_ref(st.float8_data, st.scale_reciprocal, Bm, A, ls, chunks)
        q, sc, rc = run_fuse(ops, dev, st, Bm, A, ls, chunks)
        bad = byte_mismatch(q, q_ref, E4M3)
        total += int(bad.sum())
        print(f"lora_fuse exact N={N} K={K} R={R} chunks={chunks} lora_scale={ls:g}: {int(bad.sum())} mismatching bytes of {bad.numel()}, "
              f"scale {sc.item()!r} vs {s_ref.item()!r}")
        assert same_scalar(sc, s_ref) and same_scalar(rc, r_ref), f"lora_scale {ls}: scale {sc.item()!r} vs {s_ref.item()!r}, recip {rc.item()!r} vs {r_ref.item()!r}"
        assert not bool(bad.any()), f"lora_scale {ls}: first mismatches at {bad.nonzero()[:5].tolist()}"
    assert total == 0


# ---- 6. lora_fuse_f8, random adapters ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", qr.FUSE_RANDOM_CASES, ids=fmt_id)
def test_lora_fuse_random_adapters(ops, dev, case):
    """the data of test_lora_fuse under the boundary-aware gate: scale and recip equal in bits, every byte equal unless its fp64 value lies
    within the fp32 chain's worst-case error of a bf16 rounding boundary, and then within one fp8 code"""
    N, K, R, chunks, amp = case
    st, Bm, A = qr.fuse_random_inputs(N, K, R, chunks, amp)
    exp = qr.fuse_random_expected(st, Bm, A, qr.FUSE_RANDOM_SCALE, chunks)
    assert exp["share"] <= qr.AMBIGUOUS_CAP
    q, sc, rc = run_fuse(ops, dev, st, Bm, A, qr.FUSE_RANDOM_SCALE, chunks)
    d = (u8(q.cpu()) != exp["q"])
    print(f"lora_fuse random N={N} K={K} R={R} chunks={chunks} amp={amp:g}: ambiguous share {exp['share']:.4%}, {int(d.sum())} bytes differ, "
          f"{int((d & ~exp['ambiguous']).sum())} of them unambiguous; scale {sc.item()!r} vs {exp['scale'].item()!r}")
    qr.gate_fuse_random(q, sc, rc, exp, f"lora_fuse random {case}")


# ---- 7. quantising lookup table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
def test_quant_lut_act0_equals_quantize_act(ops, dev, fmt):
    """build_quant_lut(scale, fmt, act=0) == quantize_act of all 65536 patterns, bit for bit (the two kernels on the same device), and both
    follow the oracle; a NaN input gives a NaN byte"""
    x = qr.all_bf16_patterns()
    xd = x.view(-1, 8).to(dev)
    for s in qr.quant_scales(fmt):
        sd = scalar(s).to(dev)
        lut = ops.build_quant_lut(sd, fmt, act=0).cpu()
        q = u8(ops.quantize_act(xd, sd, fmt).cpu()).flatten()
        bad = byte_mismatch(lut, qr.quantize_ref(x, scalar(s), fmt), fmt)
        print(f"quant lut {FMT_NAME[fmt]} scale={s:g}: {int((lut != q).sum())} bytes differ from quantize_act, {int(bad.sum())} from the oracle")
        assert torch.equal(lut, q)
        assert not bool(bad.any())
        assert bool(qr.f8_is_nan(lut, fmt)[torch.isnan(x)].all())
