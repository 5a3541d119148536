"""CPU companion of tests/test_helper_kernels_gpu.py: proves the gates that module applies to the helper kernels.

For every op the gate is fed (a) the fp64 reference itself, (b) seeded WRONG variants of the reference (tests/helper_refs.py, `mut=`), each of
which must be rejected at the case named in its test, and (c) torch's own fp32 kernels on the same inputs, which must pass: the gates are
attainable in fp32, so a kernel that misses one is wrong and not merely single precision.
"""
import pytest
import torch
import torch.nn.functional as F

import helper_refs as hr
from parity_util import accum_noise, round_fp64_to_bf16


def rejected(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


# ---- gemv ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(hr.GEMV_MODES))
def test_gemv_gate_rejects_wrong_kernels(mode):
    w_fp8, fmt, pre_silu = hr.GEMV_MODES[mode]
    B, K, N = 5, 1040, 200
    x, w, bias = hr.gemv_inputs(B, K, N, hr.seed_of("gemv-cpu", mode))
    a, w_op, s, _ = hr.gemv_operands(x, w, w_fp8, fmt, pre_silu)
    ref = hr.gemv_ref(a, w_op, s, bias)
    noise = accum_noise(a, w_op, s)
    hr.gate_gemv(round_fp64_to_bf16(ref), ref, noise, "reference")
    # fp32 accumulation in another order (torch's) passes
    got32 = ((a.float() @ w_op.float().T) * s + bias.float()).bfloat16()
    hr.gate_gemv(got32, ref, noise, "fp32 matmul")
    for mut in ("drop_last_16", "prev_row"):  # lane 0's second trip of the k0 loop lost / activation row b - 1 for output row b
        rejected(hr.gate_gemv, round_fp64_to_bf16(hr.gemv_ref(a, w_op, s, bias, mut=mut)), ref, noise, mut)
    if pre_silu:
        a2, w2, s2, _ = hr.gemv_operands(x, w, w_fp8, fmt, pre_silu, mut="silu_unrounded")
        rejected(hr.gate_gemv, round_fp64_to_bf16(hr.gemv_ref(a2, w2, s2, bias)), ref, noise, "silu_unrounded")


def test_gemv_small_cases_are_pooled():
    for K, N, B, mode, opts in hr.GEMV_CASES:
        assert hr.gemv_reps(B, N) * B * N >= 400


# ---- groupnorm -----------------------------------------------------------------------------------------------------------------
def _gn_fp32(x, ga, be, swish):
    y = F.group_norm(x.float().permute(0, 2, 1), 32, ga.float(), be.float(), eps=1e-6)
    if swish:
        y = y * torch.sigmoid(y)
    return y.permute(0, 2, 1).bfloat16()


def _gn_fp32_direct(x, ga, be, swish):
    """(x - mean) * rstd * gamma + beta, every step in fp32, in the kernel's order of operations"""
    B, P, C = x.shape
    v = x.float().view(B, P, 32, C // 32)
    mean = v.mean((1, 3), keepdim=True)
    rstd = torch.rsqrt(((v - mean) ** 2).mean((1, 3), keepdim=True) + 1e-6)
    y = ((v - mean) * rstd).view(B, P, C) * ga.float() + be.float()
    return (y * torch.sigmoid(y) if swish else y).bfloat16()


@pytest.mark.parametrize("C,P,swish", hr.GROUPNORM_CASES)
def test_groupnorm_gate_is_attainable_in_fp32(C, P, swish):
    x, ga, be = hr.groupnorm_inputs(3, P, C, hr.seed_of("gn", C, P, swish))
    ref = hr.groupnorm_ref(x, ga, be, swish)
    hr.gate_groupnorm(ref, ref, "reference")
    hr.gate_groupnorm(_gn_fp32_direct(x, ga, be, swish), ref, f"fp32 C={C} P={P}")
    if P * (C // 32) > 1:
        # a group of ONE value has variance 0 and rstd = 1000: ATen folds the statistics into x * (rstd gamma) + (beta - mean rstd gamma), which
        # cancels two terms 1000 times the result there (88 % bit-exact); the kernel's (x - mean) * rstd is exactly 0, as in the line above
        hr.gate_groupnorm(_gn_fp32(x, ga, be, swish), ref, f"F.group_norm fp32 C={C} P={P}")


@pytest.mark.parametrize("r", hr.GROUPNORM_OFFSETS)
def test_groupnorm_offset_gate_is_attainable_in_fp32(r):
    """the required behaviour of the kernel at large DC offsets is that of torch's fp32 group_norm: it passes the gate at |mean| / std = r"""
    for swish in (True, False):
        x, ga, be = hr.groupnorm_inputs(3, 1025, 128, hr.seed_of("gn-offset", r), offsets=r)
        ref = hr.groupnorm_ref(x, ga, be, swish)
        hr.gate_groupnorm(_gn_fp32(x, ga, be, swish), ref, f"F.group_norm fp32 offset {r}")
        # and it is sharp there: a relative error of 2^-7 in rstd, or another batch's statistics, do not pass
        for mut in ("rstd_rel_2^-7", "stats_of_batch_0"):
            rejected(hr.gate_groupnorm, hr.groupnorm_ref(x, ga, be, swish, mut=mut), ref, mut)


@pytest.mark.parametrize("mut,C,P", [("drop_pixel_511", 32, 513), ("drop_pixel_511", 128, 513), ("stats_of_batch_0", 128, 513),
                                     ("stats_of_batch_0", 2048, 1), ("group_c_div_8", 96, 513), ("group_c_div_8", 96, 1025),
                                     ("rstd_rel_2^-7", 256, 512), ("rstd_rel_2^-7", 32, 511)])
def test_groupnorm_gate_rejects_wrong_kernels(mut, C, P):
    for swish in (True, False):
        x, ga, be = hr.groupnorm_inputs(3, P, C, hr.seed_of("gn", C, P, swish))
        ref = hr.groupnorm_ref(x, ga, be, swish)
        rejected(hr.gate_groupnorm, hr.groupnorm_ref(x, ga, be, swish, mut=mut), ref, mut)


# ---- softmax_rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", hr.SOFTMAX_SCALES)
@pytest.mark.parametrize("cols", hr.SOFTMAX_COLS)
def test_softmax_gate(cols, scale):
    S = hr.softmax_inputs(cols, hr.seed_of("softmax", cols))
    ref = hr.softmax_ref(S, scale)
    assert ref[4, cols // 3] == 0 and torch.isfinite(ref.float()).all()
    tiny = torch.finfo(torch.bfloat16).tiny
    assert ((ref == 0) | (ref.float() >= tiny)).all(), "the inputs keep every probability out of the subnormals (or exactly 0)"
    hr.gate_softmax(ref, ref, "reference")
    hr.gate_softmax(torch.softmax(S.float() * scale, -1).bfloat16(), ref, f"torch.softmax fp32 cols={cols}")
    rejected(hr.gate_softmax, hr.softmax_ref(S, scale, mut="scale_sign_after_max"), ref, "scale sign")
    if cols == 2056:  # thread 0's second trip of the 2048-element loop lost
        rejected(hr.gate_softmax, hr.softmax_ref(S, scale, mut="first_2048_only"), ref, "first 2048 only")


# ---- row_norm ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rms,kind", hr.ROW_NORM_KINDS)
@pytest.mark.parametrize("D", hr.ROW_NORM_DS)
def test_row_norm_gate(D, rms, kind):
    x, w, b = hr.row_norm_inputs(D, rms, kind, hr.seed_of("row_norm", D, kind))
    eps = 1e-6 if rms else 1e-5
    ref = hr.row_norm_ref(x, w, b, eps, rms)
    hr.gate_row_norm(ref, ref, "reference")
    if rms:
        h = (x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + eps)).bfloat16()
        hr.gate_row_norm(w * h, ref, f"fp32 T5LayerNorm D={D} {kind}")
        if D >= 64:  # statistical (double roundings): needs more than a handful of values
            rejected(hr.gate_row_norm, hr.row_norm_ref(x, w, b, eps, rms, mut="weight_before_rounding"), ref, "weight before rounding")
        if kind == "rms_1e-3":  # eps matters here: dropping it is not within the gate
            rejected(hr.gate_row_norm, hr.row_norm_ref(x, w, b, 0.0, rms), ref, "no eps")
    else:
        hr.gate_row_norm(F.layer_norm(x.float(), (D,), w.float(), b.float(), eps).bfloat16(), ref, f"F.layer_norm fp32 D={D} {kind}")
        if kind == "ln_mean100":
            d = (x.double() - x.double().mean(-1, keepdim=True)).abs()
            assert ((d == 0) | (d > 2.0 ** -8)).all()  # every x is exactly the row mean (y = 0 in any arithmetic) or well away from it
            rejected(hr.gate_row_norm, hr.row_norm_ref(x, w, b, eps, rms, mut="var_without_mean"), ref, "variance without the mean")


# ---- act_mul -------------------------------------------------------------------------------------------------------------------
def test_act_quick_gelu_gate():
    x, a, _ = hr.act_sweep_inputs(None)
    ref = hr.act_mul_ref(a, None)
    assert hr.gate_act(ref, ref, None, "reference") < 0.01
    hr.gate_act((a.float() * torch.sigmoid(1.702 * a.float())).bfloat16(), ref, None, "fp32 quick_gelu")
    rejected(hr.gate_act, (a.float() * torch.sigmoid(1.6 * a.float())).bfloat16(), ref, None, "sigmoid(1.6 a)")


@pytest.mark.parametrize("b_kind", [1.0, -3.5, "random"])
def test_act_gated_gate(b_kind):
    x, a, b = hr.act_sweep_inputs(b_kind)
    ref = hr.act_mul_ref(a, b)
    assert hr.gate_act(ref, ref, b, "reference") < 0.01, "share of inputs left out as non-finite"
    rejected(hr.gate_act, hr.act_mul_ref(a, b, mut="erf_gelu"), ref, b, "erf GELU")
    if b_kind == 1.0:
        # why the reference carries gelu_tanh_f's documented fp32 rounding of tanh: ATen's own fp32 kernel passes the gate with it and misses
        # it (99.76 % bit-exact: the cancelling tail a < -3) against the unrounded function; test_act_mul pins the kernel to the former
        aten = F.gelu(a.float(), approximate="tanh").bfloat16()
        hr.gate_act(aten, ref, b, "ATen fp32 tanh GELU")
        rejected(hr.gate_act, aten, round_fp64_to_bf16(hr.gelu_new_exact64(a.double())), b, "ATen vs the unrounded gelu_new")
    if b_kind != 1.0:  # times 1 the second rounding changes nothing
        rejected(hr.gate_act, hr.act_mul_ref(a, b, mut="no_rounding_before_mul"), ref, b, "no rounding before the multiply")


# ---- attention -----------------------------------------------------------------------------------------------------------------
MUTS = {"t5": ("key_L_admitted", "key_L-1_dropped", "bias_query_minus_key", "heads_exchanged"),
        "clip": ("key_L_admitted", "key_L-1_dropped", "causal_off_by_one", "heads_exchanged")}


@pytest.mark.parametrize("style", ["t5", "clip"])
@pytest.mark.parametrize("L", hr.ATTN_LS)
def test_attention_gate_rejects_wrong_kernels(L, style):
    H = 3
    q, k, v, rel, vb, scale, causal = hr.attention_inputs(L, H, 64, style, hr.seed_of("attn-cpu", L, style), pad_random=True)
    q, k, v = q[0], k[0], v[0]
    ref = hr.attention_ref(q, k, v, L, H, 64, scale, causal, rel, vb)
    ok, worst = hr.attention_gate(round_fp64_to_bf16(ref), ref)
    assert ok and worst < 0.75, "the reference rounded to bf16 passes with room"
    for mut in MUTS[style]:
        if (mut == "key_L_admitted" and L == q.shape[0]) or (mut == "key_L-1_dropped" and L == 1):
            continue  # no such key
        if causal and mut == "key_L_admitted":
            continue  # a causal kernel never looks past the diagonal: key L is masked for every query < L
        if L == 1 and mut in ("bias_query_minus_key", "causal_off_by_one"):
            continue  # one query, one key: key - query = 0 either way, and there is no key past the diagonal
        got = hr.attention_ref(q, k, v, L, H, 64, scale, causal, rel, vb, mut=mut)
        ok, worst = hr.attention_gate(round_fp64_to_bf16(got), ref)
        assert not ok, f"{mut} at L={L} passes the gate (worst err/tol {worst:.2f})"
