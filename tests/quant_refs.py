"""References, inputs, case tables and wrong variants for the fp8 quantise family of csrc/elementwise.hip -- quantize_act, amax,
quantize_weight, dequant, build_quant_lut(act=0) and the LoRA re-fuse chain behind fluxmi_lora_fuse_f8 (dequant -> lora_delta -> axpy_f32 ->
amax_f32_as_bf16 -> weight_scale -> quantize_f32) -- shared by tests/test_quant_kernels_gpu.py (kernel vs reference) and
tests/test_quant_refs_cpu.py (each reference equals the oracle call it restates; each case rejects the wrong variants listed for it).

Every reference is elementwise torch on the CPU and calls oracle/flux_oracle.py, so the gate is equality of bits.  Rounding points:
  quantize_act     bf16(x * scale) (the product is taken in fp32 and rounded once), clamp to +-max, RNE cast to fp8   fo.to_fp8_saturated
  amax             none: max |x| over bf16 values is exact.  NaN elements are skipped (the pinned contract of fluxmi_amax); torch propagates
  quantize_weight  amax as above; scale = fp32(1 / max(amax, 1e-12)) * max_val, capped at max_val (two roundings, Tensor.__rtruediv__);
                   recip = fp32(1 / scale); then quantize_act                                                          fo.quantize_weight
  dequant          fp32(float(q) * recip): one rounding                                                 fo.F8LinearState.dequantized_weight
  lora_fuse_f8     delta: fp32 products and sums (exact on the inputs of section "exact adapters", any order); fp32(w + delta); bf16 of that;
                   amax of the bf16 values; then quantize_weight's scale and cast                       fo.lora_delta + fo.quantize_weight
  quant lut        act = 0: the quantize_act of the bf16 pattern itself

Where NaN is expected only NaN-ness is compared (any NaN encoding of the format passes, no finite byte does): `byte_mismatch`, `f32_mismatch`.

Exact adapters: lora_B = integers in [-8, 8] * 2^-6, lora_A = integers in [-8, 8] * 2^-5, lora_scale in {1, 0.5, -0.25, 0}: every product is an
integer times 2^-11, a row's magnitudes sum to at most 128 * 64 * 4 < 2^24 of these units, so every partial sum is exact in fp32 in ANY order
and the kernel's fma chain, torch's mm and an fp64 product give the same bits.

Random adapters (the data of test_lora_fuse): the gate knows which elements may differ.  With v = dequant + delta in fp64, an element is
AMBIGUOUS when v lies within (R + 3) * 2^-24 * (|lora_scale| * |B| |A| + |w|) of a bf16 rounding boundary: the worst-case error of an fp32
chain of R fmas, the scale, and the additions (derived, not measured).  scale and recip must be equal in bits, every unambiguous byte equal,
an ambiguous byte within one fp8 code.  Measured ambiguous shares with this bound (tests/test_quant_refs_cpu.py asserts <= 1 % and prints
them): 0.31 % at (N, K, R, chunks) = (384, 256, 16, 1), 0.62 % at (384, 264, 16, 3), 0.11 % at (384, 264, 4, 1), and 0.13 % at
(384, 264, 16, 3) with ten times the weights.  R = 128 would mark 13 %, so that rank is tested with exact adapters only.

The scale cap: weights of amplitude 0.05 (the model's, and test_lora_fuse's) keep amax below 1 even with a dominant element planted, and
then scale = min(448 / amax, 448) = 448 whatever amax_f32_as_bf16 returns.  Both fuse tables therefore carry cases with larger weights
(FUSE_EXACT_AMP, the last of FUSE_RANDOM_CASES), where the re-fused scale depends on the amax and "amax_before_bf16" shows.

The sign of zero: the reference sums the chunks of a fused-qkv adapter from zeros, so at lora_scale = 0 its delta is +0 and a weight of -0
re-quantises to +0.  "sum_from_first_chunk" keeps the -0; the largest exact case holds such a weight.

`mut=` selects a deliberately WRONG variant; mut=None is the reference.  A case lists the variants it must reject: a variant that cannot
change a case by construction (ld_in for the output where both strides are equal; lora_scale twice at lora_scale = 1) is not listed there.
"clamp_before_round" is listed nowhere: bf16 rounding is monotone and +-max are bf16 values, so clamp(bf16(p)) == bf16(clamp(p)) for every
fp32 product p -- it is the same function, which the CPU module proves over all 65536 inputs at every scale.
"""
import functools

import torch

import flux_oracle as fo
from helper_refs import seed_of
from parity_util import f8_ord, round_fp64_to_bf16

E4M3, E5M2 = 0, 1
FMTS = (E4M3, E5M2)
F8T = {E4M3: torch.float8_e4m3fn, E5M2: torch.float8_e5m2}
F8MAX = {E4M3: 448.0, E5M2: 57344.0}
FMT_NAME = {E4M3: "e4m3", E5M2: "e5m2"}
OUT_SENTINEL = 0x5B  # the byte that fills fp8 output a kernel must not write
HUGE = 3e38

# grid caps of the launchers (csrc/stream_view.h grid_for: 4096 workgroups of 256 threads; amax / amax_f32_as_bf16: 1024)
QUANT_TRIP = 4096 * 256  # eight-element vectors per trip of quantize_act
AMAX_TRIP = 1024 * 256  # vectors per trip of amax
FLAT_TRIP = 4096 * 256 * 4  # elements per trip of dequant / axpy_f32 / quantize_f32


def scalar(v):
    return torch.tensor(float(v), dtype=torch.float32)


def u8(t):
    return t.contiguous().view(torch.uint8)


def f32_bits(t):
    return t.contiguous().view(torch.int32)


def f8_is_nan(b, fmt):
    return torch.isnan(u8(b).view(F8T[fmt]).float())


def byte_mismatch(got, exp, fmt):
    """bool mask of fp8 bytes that differ from the expectation; where a NaN is expected any NaN encoding of the format passes"""
    got, exp = u8(got.cpu()), u8(exp)
    en = f8_is_nan(exp, fmt)
    return torch.where(en, ~f8_is_nan(got, fmt), got != exp)


def f32_mismatch(got, exp):
    got, exp = got.cpu(), exp
    en = torch.isnan(exp)
    return torch.where(en, ~torch.isnan(got), f32_bits(got) != f32_bits(exp))


def all_bf16_patterns():
    """the 65536 bf16 bit patterns in order: NaNs, infinities, -0 and the subnormals included"""
    return torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)


def quant_scales(fmt):
    return (1.0, F8MAX[fmt], 2.0 ** -20, 0.0123)


# ---- quantize_act ----------------------------------------------------------------------------------------------------------------
QUANT_VALUE_MUTS = ("no_product_rounding", "truncate_bf16", "truncate_fp8", "nan_to_max")


def quantize_ref(x, scale, fmt, mut=None):
    """x bf16 (any shape), scale a 0-dim fp32 tensor -> the fp8 bytes (uint8, x's shape)"""
    mx, f8 = F8MAX[fmt], F8T[fmt]
    if mut == "clamp_before_round":  # the same function (module docstring)
        t = (x.float() * scale).clamp(-mx, mx).bfloat16()
    elif mut == "no_product_rounding":  # fp8 straight from the fp32 product
        t = (x.float() * scale).clamp(-mx, mx)
    elif mut == "truncate_bf16":  # the product chopped to bf16
        t = (f32_bits(x.float() * scale) & -65536).view(torch.float32).clamp(-mx, mx)
    else:
        t = fo.to_fp8_saturated(x, scale, mx)
    if mut == "nan_to_max":  # an fminf / fmaxf clamp drops the NaN
        t = torch.where(torch.isnan(t), torch.full_like(t, mx), t)
    b = u8(t.to(f8))
    if mut == "truncate_fp8":  # the cast chopped: one code towards zero wherever RNE went up
        up = b.view(f8).float().abs() > t.float().abs()
        b = torch.where(up, b - 1, b)
    return b


# (cols, rows, ld_in, ld_out, column offset in, column offset out): ld_in != ld_out, both > cols, offsets multiples of 8
QUANT_STRIDE_CASES = [(8, 37, 24, 40, 8, 16), (72, 37, 104, 88, 16, 8), (264, 37, 280, 296, 8, 24)]
GUARD_ROWS = 2


def gap_fill(rows, ld):
    """what the columns around a view and the guard rows below it hold: NaN and 3e38 in turn"""
    g = torch.full((rows, ld), HUGE).bfloat16()
    g[:, ::2] = float("nan")
    return g


def quant_stride_inputs(cols, rows, ld_in, c0_in, fmt):
    """the bf16 buffer [rows + 2, ld_in]; the view is [:rows, c0_in : c0_in + cols].  Every view holds NaN, +-inf, -0 and saturating values."""
    g = torch.Generator().manual_seed(seed_of("quant-stride", cols, rows, fmt))
    x = (torch.randn(rows, cols, generator=g) * 3).bfloat16()
    x[0, 0], x[1, 1], x[2, 2], x[3, 3], x[rows - 1, cols - 1] = float("nan"), float("inf"), float("-inf"), -0.0, float("nan")
    buf = gap_fill(rows + GUARD_ROWS, ld_in)
    buf[:rows, c0_in:c0_in + cols] = x
    return buf


def quant_stride_scale(fmt):
    return scalar(F8MAX[fmt] / 6.0)  # |x| > 6 (two sigma) saturates


def quant_stride_expected(xbuf, cols, rows, ld_in, ld_out, c0_in, c0_out, scale, fmt, mut=None):
    """the whole fp8 output buffer [rows + 2, ld_out] after the call, sentinel where nothing may be written"""
    out = torch.full(((rows + GUARD_ROWS) * ld_out,), OUT_SENTINEL, dtype=torch.uint8)
    q = quantize_ref(xbuf[:rows, c0_in:c0_in + cols], scale, fmt, mut).flatten()
    ld_w = ld_in if mut == "ld_in_for_output" else ld_out
    idx = (torch.arange(rows)[:, None] * ld_w + c0_out + torch.arange(cols)[None]).flatten()
    keep = idx < out.numel()
    out[idx[keep]] = q[keep]
    return out.view(rows + GUARD_ROWS, ld_out)


BIG_ROWS, BIG_COLS = 1026, 8200  # 1,051,650 vectors: quantize_act's second trip holds the last 3074 of them (the last three rows)


@functools.lru_cache(maxsize=None)
def big_base():
    """[1026, 8200] fp32 N(0, 1), shared (read-only) by the second-trip cases of quantize_act and quantize_weight"""
    return torch.randn(BIG_ROWS, BIG_COLS, generator=torch.Generator().manual_seed(seed_of("big-base")))


@functools.lru_cache(maxsize=None)
def quant_trip2_input():
    """the last four rows carry values of their own (8 x the amplitude, an offset per row), so a lost tail or a wrapped index shows"""
    x = big_base().clone()
    x[-4:] = x[-4:] * 8 + torch.arange(1, 5, dtype=torch.float32)[:, None] * 3
    return x.bfloat16()


def quant_trip2_expected(x, scale, fmt, mut=None):
    if mut not in ("lost_second_trip", "wrapped_index"):
        return quantize_ref(x, scale, fmt, mut)
    q = quantize_ref(x, scale, fmt).view(-1, 8)
    out = q.clone()
    if mut == "wrapped_index":  # vector i of the second trip lands on vector i - QUANT_TRIP
        out[: q.shape[0] - QUANT_TRIP] = q[QUANT_TRIP:]
    out[QUANT_TRIP:] = OUT_SENTINEL
    return out.view(x.shape)


# ---- amax ------------------------------------------------------------------------------------------------------------------------
def amax_ref(xbuf, rows, cols, c0, preset=0.0, mut=None):
    """max(preset, max |x|) over the view xbuf[:rows, c0 : c0 + cols], NaN elements skipped -> 0-dim fp32"""
    if mut == "ignore_stride":  # ld = cols: rows after the first are read out of the gap
        v = xbuf.flatten()[c0:c0 + rows * cols]
    else:
        v = xbuf[:rows, c0:c0 + cols].flatten()
    if mut == "drop_last_vector":
        v = v[:-8]
    if mut == "lost_second_trip":
        v = v[: AMAX_TRIP * 8]
    v = v.float() if mut == "no_abs" else v.float().abs()
    v = v[~torch.isnan(v)]
    m = v.max() if v.numel() else scalar(0)
    return torch.maximum(scalar(preset), m)


def amax_oracle(xbuf, rows, cols, c0):
    return torch.max(torch.abs(xbuf[:rows, c0:c0 + cols])).float()  # float8_quantize.py:198,227


def _strided(x, ld, c0, fill=HUGE):
    rows, cols = x.shape
    buf = torch.full((rows + GUARD_ROWS, ld), fill).bfloat16()
    buf[:rows, c0:c0 + cols] = x
    return buf


AMAX_ROWS, AMAX_COLS = 300, 7008  # 262,800 vectors: the second trip holds the last 656, all in the last row
AMAX_TRIP2_POS = {"first": (0, 0), "last": (AMAX_ROWS - 1, AMAX_COLS - 1), "second_trip_only": (AMAX_ROWS - 1, (AMAX_TRIP + 100 - (AMAX_ROWS - 1) * (AMAX_COLS // 8)) * 8 + 3)}


@functools.lru_cache(maxsize=None)
def _amax_base():
    return torch.randn(AMAX_ROWS, AMAX_COLS, generator=torch.Generator().manual_seed(seed_of("amax-base"))).bfloat16()


def _subnormals(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(1, 0x60, (rows, cols), generator=g, dtype=torch.int32) | (torch.randint(0, 2, (rows, cols), generator=g, dtype=torch.int32) << 15)
    b[rows - 1, cols - 1] = 0x807F  # the largest subnormal, negative, in the last vector
    return b.to(torch.int16).view(torch.bfloat16)


def amax_case(name):
    """-> (xbuf, rows, cols, c0, preset, wrong variants the case rejects, nan_free).  Gaps and guard rows hold 3e38, larger than any element."""
    g = torch.Generator().manual_seed(seed_of("amax", name))
    if name.startswith("trip2_"):
        x = _amax_base().clone()
        r, c = AMAX_TRIP2_POS[name[6:]]
        x[r, c] = -64.0  # a NEGATIVE maximum; N(0, 1) stays below 7
        muts = ["ignore_stride", "no_abs"] + (["drop_last_vector"] if name == "trip2_last" else []) + (["lost_second_trip"] if name != "trip2_first" else [])
        return _strided(x, AMAX_COLS + 8, 0), AMAX_ROWS, AMAX_COLS, 0, 0.0, muts, True
    if name == "strided_gap_larger":
        x = torch.randn(9, 72, generator=g).bfloat16()
        x[8, 71] = -9.5
        return _strided(x, 104, 16), 9, 72, 16, 0.0, ["ignore_stride", "no_abs", "drop_last_vector"], True
    if name == "negative_max_dense":
        x = torch.randn(40, 64, generator=g).bfloat16()
        x[17, 5] = -11.0
        return x, 40, 64, 0, 0.0, ["no_abs"], True
    if name == "all_zero":  # +0 and -0; the pre-set 0 stays
        x = torch.zeros(6, 72).bfloat16()
        x[::2] = -0.0
        return _strided(x, 88, 8), 6, 72, 8, 0.0, ["ignore_stride"], True
    if name == "subnormals_only":
        return _strided(_subnormals(16, 64, seed_of("amax-sub")), 80, 8), 16, 64, 8, 0.0, ["ignore_stride", "no_abs", "drop_last_vector"], True
    if name == "preset_survives":
        x = torch.randn(12, 72, generator=g).bfloat16()
        return _strided(x, 88, 8), 12, 72, 8, 100.0, ["ignore_stride"], True
    if name == "preset_is_raised":
        x = torch.randn(12, 72, generator=g).bfloat16()
        x[11, 70] = -6.5
        return _strided(x, 88, 8), 12, 72, 8, 3.0, ["ignore_stride", "no_abs", "drop_last_vector"], True
    if name == "inf":
        x = torch.randn(12, 72, generator=g).bfloat16()
        x[4, 9] = float("-inf")
        return x, 12, 72, 0, 0.0, ["no_abs"], True
    if name == "nan_skipped":  # NaNs of both signs among finite values: the maximum of the others
        x = torch.randn(12, 72, generator=g).bfloat16()
        x[0, 0], x[5, 5], x[11, 71] = float("nan"), -float("nan"), float("nan")
        x[11, 69] = -8.25
        return x, 12, 72, 0, 0.0, ["no_abs", "drop_last_vector"], False
    if name == "all_nan":  # nothing but NaN: the pre-set value stays
        return torch.full((4, 16), float("nan")).bfloat16(), 4, 16, 0, 0.5, [], False
    raise KeyError(name)


AMAX_CASES = ["strided_gap_larger", "trip2_first", "trip2_last", "trip2_second_trip_only", "negative_max_dense", "all_zero", "subnormals_only",
              "preset_survives", "preset_is_raised", "inf", "nan_skipped", "all_nan"]
AMAX_MUTS = ("ignore_stride", "drop_last_vector", "no_abs", "lost_second_trip")


# ---- quantize_weight -------------------------------------------------------------------------------------------------------------
QW_SHAPES = [(1, 8), (3, 264), (BIG_ROWS, BIG_COLS)]
QW_AMPS = (1e-3, 1.0, 30.0)


def qw_positions(N, K):
    """where the dominant element goes.  Second-trip territory (past both amax's and quantize_act's first trip) exists at the large shape only."""
    pos = {"first": (0, 0), "last": (N - 1, K - 1)}
    if N * (K // 8) > QUANT_TRIP:
        pos["second_trip"] = (N - 2, 4000)  # vector 1,050,100
    elif N > 1:
        pos["middle"] = (N // 2, K // 2)
    return pos


def qw_weight(N, K, amp, pos):
    """N(0, amp) with a NEGATIVE element of four times the largest magnitude at `pos`"""
    if (N, K) == (BIG_ROWS, BIG_COLS):
        w = (big_base() * amp).bfloat16()
    else:
        w = (torch.randn(N, K, generator=torch.Generator().manual_seed(seed_of("qw", N, K))) * amp).bfloat16()
    w[pos] = -(w.abs().max() * 4)
    return w


def quantize_weight_ref(w, fmt, amax_mut=None):
    """(bytes, scale, recip); amax_mut: a wrong amax underneath"""
    if amax_mut is None:
        q, s, r = fo.quantize_weight(w, F8T[fmt])
        return u8(q), s, r
    N, K = w.shape
    s = fo.amax_to_scale(amax_ref(w, N, K, 0, mut=amax_mut), F8MAX[fmt])
    return quantize_ref(w, s, fmt), s, s.reciprocal()


# ---- dequant ---------------------------------------------------------------------------------------------------------------------
DEQ_RECIPS = (1.0, 2.0 ** -20, 0.37, 3e38)
DEQ_BIG_N = 4195328  # 1024 elements into the second trip


def dequant_bytes(n):
    """the 256 byte values tiled out to n, with a drift of one every 4099 elements: n = 256 is every byte once, and elements i and
    i + FLAT_TRIP hold different bytes (a plain tile has period 256, which divides the grid stride: a wrapped index would read the same)"""
    i = torch.arange(n, dtype=torch.int64)
    return ((i + i // 4099) & 255).to(torch.uint8)


def dequant_ref(qb, recip, fmt, mut=None):
    """qb uint8 [n] -> fp32 [n]"""
    if mut == "reverse_word_bytes":
        qb = qb.view(-1, 4).flip(1).reshape(qb.shape)
    r = recip.reciprocal() if mut == "scale_for_recip" else recip
    return qb.contiguous().view(F8T[fmt]).float().mul(r)


DEQ_MUTS = ("scale_for_recip", "reverse_word_bytes")


# ---- lora_fuse_f8 ----------------------------------------------------------------------------------------------------------------
FUSE_EXACT_CASES = [(1, 8, 1, 1), (3, 264, 16, 3), (96, 264, 128, 4), (384, 256, 16, 1), (520, 8072, 16, 3)]  # (N, K, R, chunks)
# the weight's amplitude.  At 0.05 (the model's own, and test_lora_fuse's) amax stays below 1 and the scale sits at its cap of 448 whatever
# the amax kernel returns; the other cases carry larger weights so that the re-fused scale depends on amax_f32_as_bf16.
FUSE_EXACT_AMP = {(1, 8, 1, 1): 0.05, (3, 264, 16, 3): 0.6, (96, 264, 128, 4): 0.6, (384, 256, 16, 1): 0.05, (520, 8072, 16, 3): 0.6}
FUSE_SCALES = (1.0, 0.5, -0.25, 0.0)
FUSE_MUTS = ("chunk0_always", "last_chunk_only", "drop_ragged_k", "amax_before_bf16", "rows_swapped", "lora_scale_twice", "sum_from_first_chunk")


@functools.lru_cache(maxsize=None)
def fuse_exact_inputs(N, K, R, chunks):
    """-> (st, lora_B [N, R], lora_A [chunks * R, K]): an e4m3 weight state of N(0, 0.05) and the exact-arithmetic adapters (read-only)"""
    g = torch.Generator().manual_seed(seed_of("fuse-exact", N, K, R, chunks))
    st = fo.F8LinearState((torch.randn(N, K, generator=g) * FUSE_EXACT_AMP[(N, K, R, chunks)]).bfloat16(), None)
    Bm = torch.randint(-8, 9, (N, R), generator=g).float() * 2.0 ** -6
    Bm[:, 0][Bm[:, 0] == 0] = 8 * 2.0 ** -6  # no row without an adapter (R = 1 has nothing else)
    A = torch.randint(-8, 9, (chunks * R, K), generator=g).float() * 2.0 ** -5
    return st, Bm, A


def fuse_exact_muts(N, K, R, chunks, ls):
    """the wrong variants a case must reject.  lora_scale = 0 removes the adapters: only the weight's own placement is left to get wrong."""
    muts = ["rows_swapped"] if N > 1 else []
    if ls == 0 and (N, K, R, chunks) == (520, 8072, 16, 3):  # 22 weights of -0: one of them meets three negative sums
        muts += ["sum_from_first_chunk"]
    if ls != 0:
        muts += ["chunk0_always", "last_chunk_only"] if chunks > 1 else []
        muts += ["drop_ragged_k"] if K % 256 else []
        muts += ["lora_scale_twice"] if ls != 1 else []
        muts += ["amax_before_bf16"] if N > 1 and FUSE_EXACT_AMP[(N, K, R, chunks)] > 0.05 else []
    return muts


def fuse_ref(q8, recip, Bm, A, ls, chunks, mut=None):
    """the oracle chain: (bytes, scale, recip) of requant(bf16(dequant + lora_delta)).  q8: e4m3 [N, K], A: the lora_A that is passed
    ([chunks * R, K], alpha / rank already folded in, so alpha = None)."""
    N, K = q8.shape
    deq = q8.float().mul(recip)  # fo.F8LinearState.dequantized_weight
    if mut == "rows_swapped":
        deq = deq.flip(0)
    if mut == "chunk0_always":
        A = A[: A.shape[0] // chunks].repeat(chunks, 1)
    if mut == "last_chunk_only":  # `accumulate` dropped: every chunk overwrites
        A = A[-(A.shape[0] // chunks):]
    delta = fo.lora_delta(A, Bm, None, ls)
    if mut == "sum_from_first_chunk":  # the chunk sum started from its first term, not from zeros: at lora_scale = 0 a delta of -0 survives,
        cs = A.float().chunk(chunks, 0)  # and a -0 weight keeps its sign where the reference gives +0 (the kernel did this once)
        delta = ls * torch.mm(Bm.float(), cs[0])
        for c in cs[1:]:
            delta = delta + ls * torch.mm(Bm.float(), c)
    if mut == "lora_scale_twice":
        delta = delta * ls
    if mut == "drop_ragged_k":  # the ragged last 256-column workgroup never runs
        delta[:, K // 256 * 256:] = 0
    w32 = deq + delta
    wb = w32.type(torch.bfloat16)
    if mut == "amax_before_bf16":
        s = fo.amax_to_scale(w32.abs().max(), F8MAX[E4M3])
        return quantize_ref(wb, s, E4M3), s, s.reciprocal()
    q, s, r = fo.quantize_weight(wb)
    return u8(q), s, r


# (N, K, R, chunks, weight amplitude): 0.05 is the data of test_lora_fuse (scale at its cap of 448); at 0.5 the scale depends on the amax
FUSE_RANDOM_CASES = [(384, 256, 16, 1, 0.05), (384, 264, 16, 3, 0.05), (384, 264, 4, 1, 0.05), (384, 264, 16, 3, 0.5)]
FUSE_RANDOM_SCALE, FUSE_RANDOM_ALPHA = 0.8, 8.0
FUSE_DOMINANT = (5, 7)
AMBIGUOUS_CAP = 0.01


@functools.lru_cache(maxsize=None)
def fuse_random_inputs(N, K, R, chunks, amp=0.05):
    """the data of test_lora_fuse with a dominant weight element planted as in test_quantize_weight -> (st, lora_B, the lora_A that is passed)"""
    g = torch.Generator().manual_seed(seed_of("fuse-random", N, K, R, chunks))
    w = (torch.randn(N, K, generator=g) * amp).bfloat16()
    w[FUSE_DOMINANT] = w.abs().max() * 4
    A = torch.randn(chunks * R, K, generator=g) * 0.1
    Bm = torch.randn(N, R, generator=g) * 0.1
    return fo.F8LinearState(w, None), Bm, A * FUSE_RANDOM_ALPHA / R


def bf16_boundary_distance(v):
    """fp64 v -> distance to the nearest bf16 rounding boundary (the midpoints of neighbouring bf16 values)"""
    a = v.abs()
    r = round_fp64_to_bf16(a)
    rb = r.view(torch.int16)
    up = (rb + 1).view(torch.bfloat16).double()
    dn = torch.where(rb > 0, (rb - 1).clamp_min(0).view(torch.bfloat16).double(), -up)
    r = r.double()
    return torch.minimum((a - (r + up) / 2).abs(), (a - (r + dn) / 2).abs())


def fuse_random_expected(st, Bm, A, ls, chunks):
    """-> dict(q bytes, scale, recip, ambiguous mask, share).  One bf16 rounding of the fp64 value, then the oracle's requantise."""
    R = Bm.shape[1]
    ls32 = float(scalar(ls))  # the fp32 the kernel multiplies by
    deq = st.dequantized_weight()
    Ad, Bd = A.float().double(), Bm.float().double()
    v = deq.double()
    mag = torch.zeros_like(v)
    for c in range(chunks):
        v = v + ls32 * (Bd @ Ad[c * R:(c + 1) * R])
        mag = mag + abs(ls32) * (Bd.abs() @ Ad[c * R:(c + 1) * R].abs())
    bound = (R + 3) * 2.0 ** -24 * (mag + deq.double().abs())
    amb = bf16_boundary_distance(v) <= bound
    wb = round_fp64_to_bf16(v)
    q, s, r = fo.quantize_weight(wb)
    # the scale is exact: the dominant element is unambiguous and no other element comes near it
    top2 = wb.float().abs().flatten().topk(2).values
    assert not bool(amb[FUSE_DOMINANT]) and wb[FUSE_DOMINANT].float().abs() == top2[0] and top2[1] < 0.5 * top2[0], "the dominant element does not fix the scale"
    return dict(q=u8(q), scale=s, recip=r, ambiguous=amb, share=float(amb.double().mean()))


def gate_fuse_random(got_q, got_scale, got_recip, exp, what=""):
    """scale and recip equal in bits, every unambiguous byte equal, an ambiguous byte within one fp8 code -> bytes off by one code"""
    got_q = u8(got_q.cpu())
    assert f32_bits(got_scale.cpu()).item() == f32_bits(exp["scale"]).item(), f"{what}: scale {got_scale.item()!r} vs {exp['scale'].item()!r}"
    assert f32_bits(got_recip.cpu()).item() == f32_bits(exp["recip"]).item(), f"{what}: recip {got_recip.item()!r} vs {exp['recip'].item()!r}"
    d = (f8_ord(got_q) - f8_ord(exp["q"])).abs()
    bad = (d > 0) & ~exp["ambiguous"]
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} unambiguous bytes differ"
    assert int(d.max()) <= 1, f"{what}: an ambiguous byte is {int(d.max())} fp8 codes off"
    return int((d > 0).sum())
