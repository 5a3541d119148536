"""fp64 references of the helper kernels (gemv, groupnorm, softmax_rows, row_norm, act_mul, text / vision attention) and the seeded inputs
of their tests, shared by tests/test_helper_kernels_gpu.py (kernel vs reference) and tests/test_helper_refs_cpu.py (which proves that
each gate rejects a wrong kernel and is attainable in fp32).

Every reference works in fp64 on the bf16 input VALUES and rounds only where the kernel's header comment documents a rounding:
  gemv        bf16(silu(x)) before the fp8 quantisation (csrc/gemv.hip); the result is returned unrounded
  groupnorm   one rounding at the end (csrc/vae.hip)
  softmax     one rounding at the end
  row_norm    RMS: bf16 before the weight; LayerNorm: one rounding at the end (csrc/text.hip)
  act_mul     gated: fp32 tanh before the "1 +" (gelu_tanh_f, csrc/common.h), bf16 after the GELU; quick_gelu: one rounding at the end
  attention   bf16 P, bf16 before v_bias; the result is returned unrounded

`mut=` selects a deliberately WRONG variant (the CPU module asserts that the gate rejects it); mut=None is the reference.
"""
import math

import torch

import flux_oracle as fo
from parity_util import round_fp64_to_bf16

E4M3, E5M2 = 0, 1
F8T = {E4M3: torch.float8_e4m3fn, E5M2: torch.float8_e5m2}
F8MAX = {E4M3: 448.0, E5M2: 57344.0}
SENTINEL = 0x7FC1  # a bf16 NaN payload no kernel produces: buffers a kernel must not write are filled with it and compared as bits


def rbf64(x: torch.Tensor) -> torch.Tensor:
    """fp64 -> the nearest bf16 value (one rounding), kept in fp64"""
    return round_fp64_to_bf16(x).double()


def sentinel_like(shape, device="cpu"):
    return torch.full(shape, SENTINEL, dtype=torch.int16, device=device).view(torch.bfloat16)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


def all_finite_bf16() -> torch.Tensor:
    x = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    return x[torch.isfinite(x)]


# ---- gemv ------------------------------------------------------------------------------------------------------------------------
def gemv_inputs(B, K, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, K, generator=g).bfloat16()
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16()
    bias = torch.randn(N, generator=g).bfloat16()
    return x, w, bias


def gemv_operands(x, w, w_fp8, act_fmt, pre_silu, mut=None):
    """The operands the kernel multiplies: (a [B,K], w_op [N,K], s, extras) with out = (a . w_op) * s + bias.
    fp8: w_op = e4m3 weight, a = fp8(bf16(silu(x)) * in_scale); extras = (in_scale, sa_recip, sb_recip) as fp32 scalars."""
    a = x.double()
    if pre_silu:
        a = a / (1.0 + torch.exp(-a))
        if mut != "silu_unrounded":
            a = rbf64(a)
    if not w_fp8:
        return a, w, 1.0, None
    w8, _, sb_recip = fo.quantize_weight(w)
    in_scale = fo.amax_to_scale(a.abs().max().float(), F8MAX[act_fmt])
    if mut == "silu_unrounded":  # x * scale without the bf16 rounding of silu(x) first; the product itself still rounds to bf16
        a8 = rbf64(a * in_scale.double()).clamp(-F8MAX[act_fmt], F8MAX[act_fmt]).float().to(F8T[act_fmt])
    else:
        a8 = fo.to_fp8_saturated(a.bfloat16(), in_scale, F8MAX[act_fmt]).to(F8T[act_fmt])
    sa_recip = in_scale.reciprocal()
    return a8, w8, float(sa_recip.double() * sb_recip.double()), (in_scale, sa_recip, sb_recip)


def gemv_ref(a, w_op, s, bias, mut=None):
    """fp64, unrounded: [B, N]"""
    a, w_op = a.double(), w_op.double()
    if mut == "drop_last_16":
        a = a.clone()
        a[:, -16:] = 0
    if mut == "prev_row":
        a = torch.roll(a, 1, 0)
    out = (a @ w_op.T) * s
    return out if bias is None else out + bias.double()


# ---- groupnorm -------------------------------------------------------------------------------------------------------------------
def groupnorm_inputs(B, P, C, seed, offsets=None):
    """x [B, P, C] bf16.  offsets=None: the data of test_groupnorm (std 2, mean 0.5).  offsets = r: std 1 and a mean per GROUP of r times a
    factor that cycles over (1, -1, 0.75, -0.5), so that neighbouring groups carry different DC offsets and the worst has |mean| / std = r."""
    g = torch.Generator().manual_seed(seed)
    if offsets is None:
        x = torch.randn(B, P, C, generator=g) * 2 + 0.5
    else:
        cpg = C // 32
        f = torch.tensor([1.0, -1.0, 0.75, -0.5]).repeat(8).repeat_interleave(cpg)
        x = torch.randn(B, P, C, generator=g) + float(offsets) * f
    ga = (1 + 0.1 * torch.randn(C, generator=g)).bfloat16()
    be = (0.1 * torch.randn(C, generator=g)).bfloat16()
    return x.bfloat16(), ga, be


def groupnorm_ref(x, gamma, beta, swish, eps=1e-6, mut=None):
    B, P, C = x.shape
    cpg = C // 32
    xd = x.double()
    gidx = torch.arange(C) // (8 if mut == "group_c_div_8" else cpg)  # the wrong one: c / 8 (C = 96: 12 'groups' of 8)
    ng = int(gidx.max()) + 1
    mean = torch.zeros(B, C, dtype=torch.float64)
    var = torch.zeros(B, C, dtype=torch.float64)
    for gi in range(ng):
        sel = gidx == gi
        v = xd[:, :, sel]
        if mut == "drop_pixel_511":  # the last pixel of the first 512-pixel chunk never reaches the sums
            v = torch.cat((v[:, :511], v[:, 512:]), 1)
        m = v.mean((1, 2))
        mean[:, sel] = m[:, None]
        var[:, sel] = ((v - m[:, None, None]) ** 2).mean((1, 2))[:, None]
    rstd = 1.0 / torch.sqrt(var + eps)
    if mut == "stats_of_batch_0":
        mean, rstd = mean[:1].expand(B, C), rstd[:1].expand(B, C)
    if mut == "rstd_rel_2^-7":
        rstd = rstd * (1 + 2.0 ** -7)
    y = (xd - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double()
    if swish:
        y = y / (1.0 + torch.exp(-y))
    return round_fp64_to_bf16(y)


# ---- softmax_rows ----------------------------------------------------------------------------------------------------------------
def softmax_inputs(cols, seed):
    """5 rows: Gaussian x 6 (two of them), a constant row, a row with one value 60 above the rest, a row holding one -inf.
    The spread of scale * S stays below 87: a probability under 2^-126 is a subnormal fp32, which v_exp_f32 flushes to zero, and whether the
    output keeps bf16 subnormals is not what this gate is about."""
    g = torch.Generator().manual_seed(seed)
    S = torch.randn(5, cols, generator=g) * 6
    S[2] = 3.25
    S[3] = torch.randn(cols, generator=g)
    S[3, (cols * 5) // 7] += 60.0
    S[4, cols // 3] = float("-inf")
    return S.bfloat16()


def softmax_ref(S, scale, mut=None):
    z = S.double() * scale
    if mut == "first_2048_only":  # max and sum over the first 2048 columns only
        m = z[:, :2048].max(-1, keepdim=True).values
        e = torch.exp(z - m)
        return round_fp64_to_bf16(e / e[:, :2048].sum(-1, keepdim=True))
    if mut == "scale_sign_after_max":  # exp(-scale * (S - max S)): the scale applied after the max subtraction, with the wrong sign
        e = torch.exp(-scale * (S.double() - S.double().max(-1, keepdim=True).values))
        return round_fp64_to_bf16(e / e.sum(-1, keepdim=True))
    return round_fp64_to_bf16(torch.softmax(z, -1))


# ---- row_norm --------------------------------------------------------------------------------------------------------------------
def row_norm_inputs(D, rms, kind, seed, rows=5):
    """kind: 'plain' (the data of test_row_norm), 'ln_mean100' (LayerNorm rows with mean ~100, std 1), 'rms_1e-3', 'rms_1e4'.
    ln_mean100: bf16 values near 100 sit on a grid of 0.5, and no fp32 implementation knows the row mean better than half an fp32 ulp of 100
    (3.8e-6), which is one bf16 ulp of any |y| < 1e-3.  So that the 1-ulp gate measures the kernel and not that floor, these rows take
    beta = 0 and a nominal mean of 100.25, a quarter grid step away from every x (test_helper_refs_cpu asserts that every x is the row mean itself or more than 2^-8 away)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=g) * 3 + (0.0 if rms else 1.5)
    w = (1 + 0.2 * torch.randn(D, generator=g)).bfloat16()
    b = (0.1 * torch.randn(D, generator=g)).bfloat16()
    if kind == "ln_mean100":
        x = torch.randn(rows, D, generator=g) + 100.25
        b = torch.zeros(D).bfloat16()
    elif kind == "rms_1e-3":
        x = x * 1e-3
    elif kind == "rms_1e4":
        x = x * 1e4
    else:
        assert kind == "plain"
    return x.bfloat16(), w, b


def row_norm_ref(x, w, b, eps, rms, mut=None):
    xd, wd = x.double(), w.double()
    if rms:
        h = xd * torch.rsqrt((xd * xd).mean(-1, keepdim=True) + eps)
        if mut == "weight_before_rounding":
            return round_fp64_to_bf16(wd * h)
        return round_fp64_to_bf16(wd * rbf64(h))
    mean = xd.mean(-1, keepdim=True)
    var = (xd * xd).mean(-1, keepdim=True) if mut == "var_without_mean" else ((xd - mean) ** 2).mean(-1, keepdim=True)
    return round_fp64_to_bf16((xd - mean) * torch.rsqrt(var + eps) * wd + b.double())


# ---- act_mul ---------------------------------------------------------------------------------------------------------------------
def gelu_new64(a, mut=None):
    """gelu_new with the one rounding gelu_tanh_f (csrc/common.h) documents: tanh is rounded to fp32 BEFORE the "1 +", as ATen does, so the
    cancellation of the negative tail (a < -3; -0 below -5.2) belongs to the operation and is not an error of the kernel.  test_act_mul pins
    that behaviour: it compares with the literal fp32 formula at 1 ulp."""
    if mut == "erf_gelu":
        return 0.5 * a * (1.0 + torch.erf(a / math.sqrt(2.0)))
    t = torch.tanh(0.7978845608028654 * (a + 0.044715 * a ** 3))
    return 0.5 * a * (1.0 + t.float().double())


def gelu_new_exact64(a):
    """the same function without any rounding, in the form that does not cancel: 0.5 a (1 + tanh u) = a / (1 + exp(-2u))"""
    return a / (1.0 + torch.exp(-2.0 * 0.7978845608028654 * (a + 0.044715 * a ** 3)))


def act_sweep_inputs(b_kind):
    """Every finite bf16 value as `a`, padded with zeros to a multiple of 8 per row, as [R, 8] (quick_gelu: b_kind=None) or the gated
    layout [R, 16] = [a | b] with b = 1, -3.5 or a seeded random bf16.  Returns (x, a, b)."""
    a = all_finite_bf16()
    a = torch.cat((a, torch.zeros((-a.numel()) % 8, dtype=torch.bfloat16))).reshape(-1, 8)
    if b_kind is None:
        return a, a, None
    if b_kind == "random":
        b = (torch.randn(a.shape, generator=torch.Generator().manual_seed(77)) * 2).bfloat16()
    else:
        b = torch.full(a.shape, float(b_kind)).bfloat16()
    return torch.cat((a, b), 1).contiguous(), a, b


def act_mul_ref(a, b, mut=None):
    """fp64 result rounded to bf16 once more where the kernel does; non-finite where the mathematical result overflows bf16"""
    ad = a.double()
    if b is None:
        return round_fp64_to_bf16(ad / (1.0 + torch.exp(-1.702 * ad)))
    gl = gelu_new64(ad, mut)
    if mut != "no_rounding_before_mul":
        gl = rbf64(gl)
    return round_fp64_to_bf16(gl * b.double())


# ---- attention -------------------------------------------------------------------------------------------------------------------
def attention_inputs(L, H, D, style, seed, B=1, bias_extra=0, pad_random=False):
    """Zero-padded q, k, v [B, Lp, H*D] (rows >= L zero; pad_random=True: random rows there, for the CPU mutants), rel_bias [H, 2*Lp + bias_extra] fp32 (T5) or None, v_bias [H*D] (CLIP / vision)
    or None, scale, causal."""
    g = torch.Generator().manual_seed(seed)
    Lp = (L + 31) // 32 * 32
    t5 = style == "t5"
    q, k, v = (torch.zeros(B, Lp, H * D) for _ in range(3))
    n = Lp if pad_random else L
    q[:, :n] = torch.randn(B, n, H * D, generator=g) * (0.35 if t5 else 1.0)
    k[:, :n] = torch.randn(B, n, H * D, generator=g) * (0.35 if t5 else 1.0)
    v[:, :n] = torch.randn(B, n, H * D, generator=g)
    # the last valid key dominates some queries at every L, the last query among them (the only one that sees it under a causal mask): a
    # kernel that drops it cannot hide in a 1 / L share
    if L > 1:
        q[:, L - 1] = 0.5 * k[:, L - 1]
    k[:, L - 1] *= 4
    rel = torch.randn(H, 2 * Lp + bias_extra, generator=g) if t5 else None
    vb = None if t5 else (0.3 * torch.randn(H * D, generator=g)).bfloat16()
    scale = 1.0 if t5 else (0.125 if D == 64 else 72 ** -0.5)
    return q.bfloat16(), k.bfloat16(), v.bfloat16(), rel, vb, scale, style == "clip"


def poison(t, L, dim):
    """a copy of t with the slices >= L along `dim` filled with +-1.0e4 (finite: 0 * inf in the P V MFMA would be NaN by construction)"""
    t = t.clone()
    idx = [slice(None)] * t.ndim
    idx[dim] = slice(L, None)
    sub = t[tuple(idx)]
    sign = torch.where((torch.arange(sub.numel()) % 3 == 0).reshape(sub.shape), -1.0, 1.0)
    t[tuple(idx)] = (1.0e4 * sign).to(t.dtype)
    return t


def attention_ref(q, k, v, L, H, D, scale, causal, rel=None, vb=None, mut=None):
    """q, k, v [Lp, H*D] bf16 (one sequence; rows >= L are padding the kernel must ignore) -> fp64 [L, H*D], unrounded."""
    nk = L + 1 if mut == "key_L_admitted" else (L - 1 if mut == "key_L-1_dropped" else L)
    assert nk <= q.shape[0]
    qh = q[:L].double().view(L, H, D).transpose(0, 1)
    kh = k[:nk].double().view(nk, H, D).transpose(0, 1)
    vh = v[:nk].double().view(nk, H, D).transpose(0, 1)
    if mut == "heads_exchanged":
        vh = vh.flip(0)
    s = torch.matmul(qh, kh.transpose(-1, -2)) * scale
    qi, ki = torch.arange(L)[:, None], torch.arange(nk)[None, :]
    if rel is not None:
        d = (qi - ki) if mut == "bias_query_minus_key" else (ki - qi)
        s = s + rel.double()[:, d + rel.shape[1] // 2]
    if causal:
        s = s.masked_fill(ki > qi + (1 if mut == "causal_off_by_one" else 0), float("-inf"))
    p = rbf64(torch.softmax(s, -1))
    o = torch.matmul(p, vh).transpose(0, 1).reshape(L, H * D)
    if vb is not None:
        o = rbf64(o) + vb.double()
    return o


def attention_gate(got, ref):
    """The per-element gate of test_text_attention: one bf16 ulp of the output + the bf16 rounding of P.  Returns (ok, worst err / tol)."""
    err = (got.double() - ref).abs()
    tol = 2.0 ** -8 * ref.abs().clamp(min=0.05) + 4e-3
    return bool((err <= tol).all()), float((err / tol).max())


# ---- the cases both modules walk -----------------------------------------------------------------------------------------------
# gemv: (K, N, B, mode, options).  Every K of {16, 256, 1024, 1040, 3072} and every N of {1, 15, 64, 65, 200} with at least two values of B.
# K: 16 = one lane busy; 256 = lanes 16..63 idle (the time embedder); 1024 = exactly one trip of the k0 loop; 1040 = a second trip for lane 0
# only; 3072 = production (B = 8: 96 KB of LDS).  N: 1 and 15 leave waves without rows; 65 = a second block with one row.
GEMV_MODES = {  # mode -> (w_fp8, act_fmt, pre_silu)
    "fp8_e5m2_silu": (True, E5M2, True), "fp8_e4m3_silu": (True, E4M3, True), "bf16": (False, E5M2, False), "bf16_silu": (False, E5M2, True),
}
GEMV_CASES = [
    (16, 1, 1, "fp8_e5m2_silu", ""), (16, 64, 5, "bf16_silu", "nobias"), (16, 200, 8, "fp8_e4m3_silu", "xview"),
    (256, 15, 1, "fp8_e4m3_silu", "outview"), (256, 65, 8, "fp8_e5m2_silu", "nobias xview outview"), (256, 200, 5, "bf16", ""),
    (1024, 1, 8, "bf16", "outview"), (1024, 64, 1, "fp8_e5m2_silu", ""), (1024, 15, 5, "fp8_e4m3_silu", "nobias"),
    (1040, 65, 5, "fp8_e5m2_silu", "xview outview"), (1040, 200, 1, "bf16_silu", "xview"), (1040, 15, 8, "fp8_e4m3_silu", ""),
    (3072, 64, 5, "bf16_silu", "outview"), (3072, 200, 8, "fp8_e4m3_silu", "xview outview"), (3072, 1, 1, "fp8_e5m2_silu", "nobias"),
    (3072, 65, 8, "bf16", "nobias xview"),
]

# groupnorm: (C, P, swish) at B = 3.  C = 96: c8 = 12, npl = 21, threads 252..255 idle; 128 / 256: the decoder's widths; 2048: npl = 1 (small P
# only).  P = 1, and both sides of the 512-pixel chunk.
GROUPNORM_CASES = [
    (32, 1, True), (32, 511, False), (32, 512, True), (32, 513, False), (32, 1025, True),
    (96, 1, False), (96, 511, True), (96, 513, True), (96, 1025, False),
    (128, 512, False), (128, 513, True), (128, 1025, True), (128, 1025, False),
    (256, 1, True), (256, 512, True), (256, 1025, False),
    (2048, 1, False), (2048, 511, True), (2048, 513, False),
]
GROUPNORM_OFFSETS = [0, 8, 32, 64]  # |mean| / std of the worst group, C = 128, P = 1025

SOFTMAX_COLS = [8, 2040, 2048, 2056, 4096]
SOFTMAX_SCALES = [0.125, 1.0]

ROW_NORM_DS = [8, 64, 1152, 2048, 2056, 4096]
ROW_NORM_KINDS = [(True, "plain"), (False, "plain"), (False, "ln_mean100"), (True, "rms_1e-3"), (True, "rms_1e4")]

ATTN_LS = [1, 31, 32, 33, 77, 1024]
ATTN_HS = [1, 3]
ATTN_STYLES = [("t5", 0), ("t5", 64), ("clip", 0)]  # (style, bias_ld - 2*Lp)


def seed_of(*key):
    """a stable seed per case (hash() of a str is salted per process)"""
    h = 0
    for c in repr(key):
        h = (h * 131 + ord(c)) % 1000003
    return h


# ---- the gates (one definition for both modules) -------------------------------------------------------------------------------
from parity_util import accum_noise, assert_bf16_close, assert_close_mag  # noqa: E402


def gemv_reps(B, N):
    """min_exact = 0.98 says nothing about a 1-element output: small cases are repeated with fresh seeds and gated together (>= 400 values)"""
    return max(1, -(-400 // (B * N)))


def gate_gemv(got, ref64, noise, what):
    return assert_close_mag(got, round_fp64_to_bf16(ref64), mag=noise, ulps=1, min_exact=0.98, what=what)


def gate_groupnorm(got, ref, what):
    return assert_close_mag(got, ref, mag=0.25, ulps=1, min_exact=0.99, what=what)


def gate_softmax(got, ref, what):
    return assert_bf16_close(got, ref, max_ulp=1, min_exact=0.99, what=what)


def gate_row_norm(got, ref, what):
    return assert_bf16_close(got, ref, max_ulp=1, min_exact=0.98, what=what)


def gate_act(got, ref, b, what):
    """test_act_tables' gate on the activation; for the gated product the 1e-4 floor scales with |b|.  Positions where the REFERENCE is not
    finite are left out (returns their share); the kernel must be non-finite exactly there."""
    fin = torch.isfinite(ref.float())
    assert torch.equal(torch.isfinite(got.float().cpu()), fin), f"{what}: non-finite outputs at other places than the reference"
    mag = 1e-4 if b is None else (1e-4 * b.double().abs())[fin]
    assert_close_mag(got.cpu()[fin], ref[fin], mag=mag, ulps=1, min_exact=0.999, what=what)
    return 1.0 - fin.double().mean().item()
