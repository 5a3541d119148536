"""CPU companion of tests/test_quant_kernels_gpu.py: proves the gates that module applies to the fp8 quantise family.

For every kernel (a) the reference of tests/quant_refs.py equals the oracle call it restates, and (b) at every case the expected output
differs from the output of each wrong variant (`mut=`) the case lists -- a case that a listed variant leaves unchanged is too weak.  Every
variant is listed by at least one case.  For the LoRA fuse: the exact-arithmetic adapters really are exact (fp32 mm == fp64 mm), and the
random adapters' ambiguous share stays under the 1 % cap while the oracle's own fp32 chain passes the gate.
"""
import pytest
import torch

import flux_oracle as fo
import quant_refs as qr
from quant_refs import E4M3, F8MAX, F8T, FMT_NAME, FMTS, byte_mismatch, f32_bits, f32_mismatch, scalar, u8


def fmt_id(v):
    return FMT_NAME.get(v, str(v)) if isinstance(v, int) else str(v).replace(" ", "")


def same_triple(a, b, fmt=E4M3):
    return not bool(byte_mismatch(a[0], b[0], fmt).any()) and f32_bits(a[1]).item() == f32_bits(b[1]).item() and f32_bits(a[2]).item() == f32_bits(b[2]).item()


# ---- quantize_act ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
def test_quantize_ref_is_the_oracle_and_specials(fmt):
    x = qr.all_bf16_patterns()
    for s in qr.quant_scales(fmt):
        ref = qr.quantize_ref(x, scalar(s), fmt)
        assert torch.equal(ref, u8(fo.to_fp8_saturated(x, scalar(s), F8MAX[fmt]).to(F8T[fmt])))
        assert bool(qr.f8_is_nan(ref, fmt)[torch.isnan(x)].all()) and not bool(qr.f8_is_nan(ref, fmt)[~torch.isnan(x)].any())
        inf = torch.isinf(x)
        assert torch.equal(ref[inf], u8((torch.sign(x[inf].float()) * F8MAX[fmt]).to(F8T[fmt])))
        # clamping before the bf16 rounding is the same function: rounding is monotone and +-max are bf16 values
        assert not bool(byte_mismatch(qr.quantize_ref(x, scalar(s), fmt, mut="clamp_before_round"), ref, fmt).any())


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", qr.QUANT_STRIDE_CASES, ids=fmt_id)
def test_quantize_strided_cases_reject_wrong_kernels(case, fmt):
    cols, rows, ld_in, ld_out, c0_in, c0_out = case
    assert ld_in != ld_out and min(ld_in, ld_out) > cols and c0_in % 8 == 0 and c0_out % 8 == 0 and cols % 8 == 0
    xbuf = qr.quant_stride_inputs(cols, rows, ld_in, c0_in, fmt)
    scale = qr.quant_stride_scale(fmt)
    args = (xbuf, cols, rows, ld_in, ld_out, c0_in, c0_out, scale, fmt)
    exp = qr.quant_stride_expected(*args)
    # the gap and the guard rows keep the sentinel; the view is the oracle's
    view = exp[:rows, c0_out:c0_out + cols]
    assert torch.equal(view, qr.quantize_ref(xbuf[:rows, c0_in:c0_in + cols], scale, fmt))
    assert int((exp == qr.OUT_SENTINEL).sum()) >= exp.numel() - rows * cols
    for mut in qr.QUANT_VALUE_MUTS + ("ld_in_for_output",):
        assert bool(byte_mismatch(qr.quant_stride_expected(*args, mut=mut), exp, fmt).any()), mut
    # a kernel that read the gap (the view taken at the wrong column) meets NaN and 3e38
    shifted = qr.quant_stride_expected(xbuf, cols, rows, ld_in, ld_out, c0_in - 8, c0_out, scale, fmt)
    assert bool(byte_mismatch(shifted, exp, fmt).any())


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
def test_quantize_second_trip_case_rejects_wrong_kernels(fmt):
    x = qr.quant_trip2_input()
    assert x.shape[0] * (x.shape[1] // 8) > qr.QUANT_TRIP
    scale = qr.quant_stride_scale(fmt)
    exp = qr.quant_trip2_expected(x, scale, fmt)
    for mut in ("no_product_rounding", "truncate_bf16", "truncate_fp8", "lost_second_trip", "wrapped_index"):
        bad = byte_mismatch(qr.quant_trip2_expected(x, scale, fmt, mut=mut), exp, fmt)
        assert bool(bad.any()), mut
        if mut == "lost_second_trip":
            assert not bool(bad.view(-1, 8)[: qr.QUANT_TRIP].any()) and bool(bad.view(-1, 8)[qr.QUANT_TRIP:].any())


# ---- amax ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", qr.AMAX_CASES)
def test_amax_cases_reject_wrong_kernels(name):
    xbuf, rows, cols, c0, preset, muts, nan_free = qr.amax_case(name)
    exp = qr.amax_ref(xbuf, rows, cols, c0, preset)
    if nan_free:
        assert f32_bits(exp).item() == f32_bits(torch.maximum(scalar(preset), qr.amax_oracle(xbuf, rows, cols, c0))).item()
    else:  # the pinned divergence: torch propagates the NaN, the kernel's fmaxf skips it
        assert bool(torch.isnan(qr.amax_oracle(xbuf, rows, cols, c0))) and not bool(torch.isnan(exp))
    for mut in muts:
        assert f32_bits(qr.amax_ref(xbuf, rows, cols, c0, preset, mut=mut)).item() != f32_bits(exp).item(), mut


def test_amax_cases_cover_every_variant_and_the_second_trip():
    listed = set()
    for name in qr.AMAX_CASES:
        listed |= set(qr.amax_case(name)[5])
    assert listed == set(qr.AMAX_MUTS)
    assert qr.AMAX_ROWS * (qr.AMAX_COLS // 8) > qr.AMAX_TRIP
    r, c = qr.AMAX_TRIP2_POS["second_trip_only"]
    assert r * (qr.AMAX_COLS // 8) + c // 8 >= qr.AMAX_TRIP and (r, c) != qr.AMAX_TRIP2_POS["last"]
    assert qr.amax_case("all_zero")[0][:6, 8:80].float().abs().max() == 0 and qr.amax_ref(*qr.amax_case("all_zero")[:5]).item() == 0.0
    sub = qr.amax_case("subnormals_only")
    assert 0 < qr.amax_ref(*sub[:5]).item() < 2.0 ** -126
    assert qr.amax_ref(*qr.amax_case("preset_survives")[:5]).item() == 100.0 and qr.amax_ref(*qr.amax_case("all_nan")[:5]).item() == 0.5
    assert qr.amax_ref(*qr.amax_case("inf")[:5]).item() == float("inf")


# ---- quantize_weight -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("shape", qr.QW_SHAPES, ids=fmt_id)
def test_quantize_weight_cases(shape, fmt):
    N, K = shape
    pos = qr.qw_positions(N, K)
    if N * (K // 8) > qr.QUANT_TRIP:
        r, c = pos["second_trip"]
        assert r * (K // 8) + c // 8 >= qr.QUANT_TRIP > qr.AMAX_TRIP
    for amp in qr.QW_AMPS:
        for where, p in pos.items():
            w = qr.qw_weight(N, K, amp, p)
            ref = qr.quantize_weight_ref(w, fmt)
            # the restatement (amax_ref -> amax_to_scale -> quantize_ref) is fo.quantize_weight
            s = fo.amax_to_scale(qr.amax_ref(w, N, K, 0), F8MAX[fmt])
            assert same_triple((qr.quantize_ref(w, s, fmt), s, s.reciprocal()), ref, fmt)
            assert ref[1].item() == min(F8MAX[fmt], ref[1].item())
            if amp >= 1:  # below, the scale sits at its cap whatever the amax: the case is there for the cap
                muts = ["no_abs"] + (["drop_last_vector"] if where == "last" else []) + (["lost_second_trip"] if where in ("second_trip", "last") and N > 1000 else [])
                for mut in muts:
                    assert not same_triple(qr.quantize_weight_ref(w, fmt, amax_mut=mut), ref, fmt), (amp, where, mut)
            else:
                assert ref[1].item() == F8MAX[fmt]
    z = qr.quantize_weight_ref(torch.zeros(N, K).bfloat16(), fmt)
    assert z[1].item() == F8MAX[fmt] and not bool(z[0].any())


# ---- dequant ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("n", [256, qr.DEQ_BIG_N])
def test_dequant_cases_reject_wrong_kernels(n, fmt):
    qb = qr.dequant_bytes(n)
    assert n % 4 == 0 and sorted(set(qb[:256].tolist())) == list(range(256))
    if n > qr.FLAT_TRIP:  # a wrapped index reads another byte
        assert bool((qb[qr.FLAT_TRIP:] != qb[: n - qr.FLAT_TRIP]).all())
    st = fo.F8LinearState(torch.zeros(1, 8).bfloat16(), None, f8=F8T[fmt])
    for recip in qr.DEQ_RECIPS:
        exp = qr.dequant_ref(qb, scalar(recip), fmt)
        st.float8_data, st.scale_reciprocal = qb.view(F8T[fmt]), scalar(recip)
        assert not bool(f32_mismatch(st.dequantized_weight(), exp).any())
        nan = qr.f8_is_nan(qb, fmt)
        assert bool(torch.isnan(exp[nan]).all()) and int(nan[:256].sum()) == (2 if fmt == E4M3 else 6)
        for mut in qr.DEQ_MUTS:
            if mut == "scale_for_recip" and recip == 1.0:
                continue  # 1 / 1: nothing to tell apart
            assert bool(f32_mismatch(qr.dequant_ref(qb, scalar(recip), fmt, mut=mut), exp).any()), (recip, mut)


# ---- lora_fuse_f8 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", qr.FUSE_EXACT_CASES, ids=fmt_id)
def test_fuse_exact_cases(case):
    N, K, R, chunks = case
    st, Bm, A = qr.fuse_exact_inputs(N, K, R, chunks)
    # the exact-arithmetic property: fp32 mm == fp64 mm, chunk by chunk and summed, at every lora_scale
    for ls in qr.FUSE_SCALES:
        d64 = sum(ls * (Bm.double() @ c.double()) for c in A.chunk(chunks, 0))
        d32 = fo.lora_delta(A, Bm, None, ls)
        assert d32.dtype == torch.float32 and torch.equal(d32.double(), d64)
        assert float(sum(Bm.double().abs() @ c.double().abs() for c in A.chunk(chunks, 0)).max()) * 2 ** 11 < 2 ** 24  # in units of 2^-11
    for c in A.chunk(chunks, 0):
        assert torch.equal(torch.mm(Bm, c).double(), Bm.double() @ c.double())
    listed = set()
    for ls in qr.FUSE_SCALES:
        ref = qr.fuse_ref(st.float8_data, st.scale_reciprocal, Bm, A, ls, chunks)
        # the restatement is the oracle's own fuse: F8LinearState.dequantized_weight + lora_delta -> set_weight_tensor
        st2 = fo.F8LinearState(torch.zeros(1, 8).bfloat16(), None)
        st2.float8_data, st2.scale, st2.scale_reciprocal = st.float8_data, st.scale, st.scale_reciprocal
        st2.set_weight_tensor((st2.dequantized_weight() + fo.lora_delta(A, Bm, None, ls)).type(torch.bfloat16))
        assert same_triple((u8(st2.float8_data), st2.scale, st2.scale_reciprocal), ref)
        if ls == 0:  # the reference's own requantise round trip of the weight
            # (but for the sign of zero: a -0 weight plus the +0 delta is +0)
            rt = fo.quantize_weight(st.dequantized_weight().bfloat16())
            keep = u8(st.float8_data) != 0x80
            assert torch.equal(ref[0][keep], u8(rt[0])[keep]) and not bool(ref[0][~keep].any()) and same_triple((ref[0], rt[1], rt[2]), ref)
        for mut in qr.fuse_exact_muts(N, K, R, chunks, ls):
            listed.add(mut)
            assert not same_triple(qr.fuse_ref(st.float8_data, st.scale_reciprocal, Bm, A, ls, chunks, mut=mut), ref), (ls, mut)
    if case == (520, 8072, 16, 3):
        assert N * K > qr.FLAT_TRIP and K % 256 == 136 and listed == set(qr.FUSE_MUTS)


@pytest.mark.parametrize("case", qr.FUSE_RANDOM_CASES, ids=fmt_id)
def test_fuse_random_gate(case):
    N, K, R, chunks, amp = case
    ls = qr.FUSE_RANDOM_SCALE
    st, Bm, A = qr.fuse_random_inputs(N, K, R, chunks, amp)
    exp = qr.fuse_random_expected(st, Bm, A, ls, chunks)
    print(f"lora_fuse random N={N} K={K} R={R} chunks={chunks} amp={amp:g}: ambiguous share {exp['share']:.4%} (cap {qr.AMBIGUOUS_CAP:.0%})")
    assert exp["share"] <= qr.AMBIGUOUS_CAP
    # the oracle's fp32 chain (torch's mm, another summation order than the kernel's) passes the gate
    q, s, r = qr.fuse_ref(st.float8_data, st.scale_reciprocal, Bm, A, ls, chunks)
    off = qr.gate_fuse_random(q, s, r, exp, "oracle fp32 chain")
    print(f"  oracle fp32 chain: {off} ambiguous bytes one code off")
    muts = ["rows_swapped", "lora_scale_twice"] + (["amax_before_bf16"] if amp > 0.05 else []) + (["chunk0_always", "last_chunk_only"] if chunks > 1 else []) + (["drop_ragged_k"] if K % 256 else [])
    for mut in muts:
        qm, sm, rm = qr.fuse_ref(st.float8_data, st.scale_reciprocal, Bm, A, ls, chunks, mut=mut)
        with pytest.raises(AssertionError):
            qr.gate_fuse_random(qm, sm, rm, exp, mut)
    # one unambiguous byte moved by one code is enough
    q1 = q.clone().flatten()
    i = int((~exp["ambiguous"]).flatten().nonzero()[17])
    q1[i] = q1[i] + (1 if (int(q1[i]) & 0x7F) < 0x7E else -1)
    with pytest.raises(AssertionError):
        qr.gate_fuse_random(q1.view(N, K), s, r, exp, "one byte")


def test_bf16_boundary_distance():
    v = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0, 1.0 - 2.0 ** -9, -(3.0 + 2.0 ** -7), 0.75], dtype=torch.float64)
    d = qr.bf16_boundary_distance(v)
    assert d.tolist() == [0.0, 2.0 ** -20, 2.0 ** -9, 0.0, 0.0, 2.0 ** -9]
