"""fp64 references of the block glue kernels (ln_modulate, qkv_rope, gate_residual, add / add_bcast, euler_, rope_table,
timestep_embedding; csrc/elementwise.hip, csrc/qkv_rope.hip), their seeded inputs, gates and case tables, shared by
tests/test_block_kernels_gpu.py (kernel vs reference) and tests/test_block_refs_cpu.py (which proves that each gate accepts the reference
and an fp32 model in the kernel's order of operations, and rejects the wrong kernels it is meant to catch).

Every reference works in fp64 on the bf16 input VALUES and rounds where the kernel's header comment documents a rounding:
  ln_modulate   bf16(bf16(bf16(1 + scale) * bf16(LN(x))) + shift), fp64 mean / variance, eps 1e-6; fp8 form fp8(clamp(bf16(y * q)))
  qkv_rope      bf16((x * rinv) * w) with the fp64 RMS over the 128 head channels, eps 1e-6, then the rotation in bf16 arithmetic:
                bf16(bf16(c x0) + bf16(-s x1)), bf16(bf16(s x0) + bf16(c x1)); K optionally fp16 OF THE bf16 VALUE; V^T bit2 <-> bit3 permuted
  gate_residual bf16(x + bf16(gate * y));  add: bf16(a + b);  euler_: bf16(img + bf16(fp32(dt * pred)))       -- exact chains, compared as bits
  rope_table / timestep_embedding   fp64 cos / sin of the fp32 product the kernel forms, rounded once

`mut=` selects a deliberately WRONG variant (the CPU module asserts that the gate rejects it); mut=None is the reference.
"""
import functools
import math

import torch

import flux_oracle as fo
from helper_refs import E4M3, E5M2, F8MAX, F8T, SENTINEL, bits, rbf64, seed_of, sentinel_like  # noqa: F401  (one definition, re-exported)
from parity_util import assert_bf16_close, assert_close_mag, assert_f8_close, bf16_ord, round_fp64_to_bf16

POOL = 4096  # min_exact needs a population: cases with fewer output values are repeated with fresh seeds and gated together
FMTS = {"bf16": None, "e5m2": E5M2, "e4m3": E4M3}
# fp8 input scales of the two streams: far apart, so that the wrong stream's scale is loud; e4m3 saturates (448) on part of the values
LN_QSCALES = {E5M2: (900.0, 20000.0), E4M3: (24.0, 150.0)}


def reps_for(n_values):
    return max(1, -(-POOL // n_values))


# ---- ln_modulate -----------------------------------------------------------------------------------------------------------------
def ln_inputs(B, L, H, seed, offset=0.0, amp=None):
    """x [B, L, H] bf16 and the modulation vectors as views of one [B, 4H] table (row stride 4H, as the engine's): shift0, scale0, shift1,
    scale1.  Default data: std 2, mean 0.3 (test_ln_modulate's).  offset = r: std 1 and a row mean of +-r (sign alternates over rows), i.e.
    |mean| / std = r.  amp: std `amp`, mean 0 (1e-3: the variance is eps itself; 1e4)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, H, generator=g)
    if amp is not None:
        x = x * amp
    elif offset:
        sign = torch.where(torch.arange(B * L).reshape(B, L, 1) % 2 == 0, 1.0, -1.0)
        x = x + offset * sign
    else:
        x = x * 2 + 0.3
    mods = (torch.randn(B, 4 * H, generator=g) * 0.5).bfloat16()
    return x.bfloat16(), mods[:, :H], mods[:, H:2 * H], mods[:, 2 * H:3 * H], mods[:, 3 * H:]


def _by_stream(L, split, v0, v1, le=False):
    """[B, H] vectors of the two streams -> [B, L, H]: rows l < split take stream 0's (le: l <= split, the wrong one)"""
    l = torch.arange(L)[None, :, None]
    return torch.where((l <= split) if le else (l < split), v0[:, None], v1[:, None])


def ln_modulate_ref(x, sh0, sc0, sh1, sc1, split, mut=None):
    """-> (y bf16 [B, L, H], mag fp64 = |(1 + scale) LN| + |shift|: the size of the terms y is the rounded sum of)"""
    B, L, H = x.shape
    xd = x.double()
    if mut == "batch_shift":  # batch b's vectors modulate batch b + 1
        sh0, sc0, sh1, sc1 = (torch.roll(t, 1, 0) for t in (sh0, sc0, sh1, sc1))
    mom = xd[..., :-8] if mut == "drop_last_8" else xd  # the last 16-byte chunk of the row never reaches the moments
    if mut == "one_pass_var":  # E[x^2] - mean^2, in fp32
        x32 = x.float()
        m32 = x32.mean(-1, keepdim=True)
        mean, var = m32.double(), ((x32 * x32).mean(-1, keepdim=True) - m32 * m32).clamp_min(0).double()
    else:
        mean = mom.mean(-1, keepdim=True)
        var = ((mom - mean) ** 2).mean(-1, keepdim=True)
    n = rbf64((xd - mean) / torch.sqrt(var + 1e-6))
    le = mut == "split_le"
    scale = _by_stream(L, split, sc0.double(), sc1.double(), le)
    shift = _by_stream(L, split, sh0.double(), sh1.double(), le)
    m1 = 1.0 + scale if mut == "scale_unrounded" else rbf64(1.0 + scale)
    t = m1 * n
    return round_fp64_to_bf16(rbf64(t) + shift), t.abs() + shift.abs()


def ln_quant_ref(y, split, q0, q1, fmt, mut=None):
    """the fp8 form of a bf16 result y [B, L, H]: fp8(clamp(bf16(y * q))) with the q of the row's stream"""
    if mut == "wrong_q_stream":
        q0, q1 = q1, q0
    out = torch.empty(y.shape, dtype=F8T[fmt])
    out[:, :split] = fo.to_fp8_saturated(y[:, :split], torch.tensor(q0), F8MAX[fmt]).to(F8T[fmt])
    out[:, split:] = fo.to_fp8_saturated(y[:, split:], torch.tensor(q1), F8MAX[fmt]).to(F8T[fmt])
    return out


def _r32(t):
    return t.bfloat16().float()


def ln_modulate_fp32(x, sh0, sc0, sh1, sc1, split, order):
    """The kernels' arithmetic in torch fp32, in their order of operations (csrc/elementwise.hip).  Lane `ln` of the wave owns the 8-column
    chunks ln, ln + 64, ...; order = "one_wave": one accumulator per lane, sequential over its elements (ln_modulate_kernel);
    "pairwise": two accumulators per lane, even and odd elements, added at the end (the packed adds of ln_modulate_stream_kernel).  Then the
    wave's xor butterfly over the 64 lane sums, twice: mean first, then the squares of x - mean."""
    B, L, H = x.shape
    nch = -(-H // 512)
    xp = torch.zeros(B, L, nch * 512)
    xp[..., :H] = x.float()
    valid = (torch.arange(nch * 512) < H).view(nch, 64, 8)
    v = xp.view(B, L, nch, 64, 8)

    def lane_reduce(vals):  # [B, L, nch, 64, 8] -> [B, L, 64] -> [B, L, 1]
        acc = [torch.zeros(B, L, 64), torch.zeros(B, L, 64)]
        for k in range(nch):
            for j in range(8):
                a = j & 1 if order == "pairwise" else 0
                acc[a] = acc[a] + vals[:, :, k, :, j]
        s = acc[0] + acc[1]
        lane = torch.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[..., lane ^ o]
        return s[..., :1]

    mean = lane_reduce(v) / float(H)
    d = torch.where(valid, v - mean[..., None, None], torch.zeros(()))
    var = lane_reduce(d * d) / float(H)
    rstd = 1.0 / torch.sqrt(var + 1e-6)
    n = _r32((x.float() - mean) * rstd)
    scale = _by_stream(L, split, sc0.float(), sc1.float())
    shift = _by_stream(L, split, sh0.float(), sh1.float())
    return (_r32(_r32(1.0 + scale) * n) + shift).bfloat16()


def gate_ln_bf16(got, ref, mag, what, min_exact=0.999):
    return assert_close_mag(got, ref, mag=mag, ulps=2, min_exact=min_exact, what=what)


def gate_ln_f8(got, ref, what, y=None, mag=None):
    """test_ln_modulate's fp8 gate: at most 1 fp8 code from the quantised reference, 0.999 identical.  With y (the bf16 reference) and mag:
    the 1-code clause is applied where |y| >= mag / 8 only; the 0.999 share is still taken over ALL values.  Where bf16((1 + scale) LN) and
    shift cancel, one bf16 ulp of the product -- which the bf16 gate allows, it measures at `mag` -- is a large relative step of y, hence
    several fp8 codes: the fp32 models of this module do that at 3 of 8.3 M values (H = 3072, shape (64, 42, 13): |y| / mag < 0.01, 2 to 8
    codes).  The bf16 gate allows 2 ulps at mag = mag * 2^-6, an fp8 code is at least 2^-3 |y| (e4m3), so |y| >= mag / 8 is where a result
    inside the bf16 gate cannot move by more than one code.  The other values (6 %) are still pinned: the GPU module requires the fp8
    output to be the quantised bf16 output of the same kernel byte for byte, and that bf16 output passes the bf16 gate."""
    if y is None:
        return assert_f8_close(got, ref, max_ulp=1, min_exact=0.999, what=what)
    well = (y.detach().cpu().double().abs() >= mag.detach().cpu().double() / 8).reshape(got.shape)
    assert_f8_close(got.cpu()[well], ref.cpu()[well], max_ulp=1, min_exact=0.999, what=what + " (|y| >= mag / 8)")
    exact = (got.cpu().view(torch.uint8) == ref.cpu().view(torch.uint8)).float().mean().item()
    assert exact >= 0.999, f"{what}: identical share {exact:.5f} over all values (need 0.999)"
    return exact


# LN_HS: both sides of every chunk count of the launcher (NCH 1 | 2 | 4 | 6 | 8 at 512-column chunks), the guard-free arms (H = NCH * 512:
# 512, 1024, 2048, 3072) next to guarded ones with a ragged last chunk (520, 3080), one lane busy (8), lanes 8..63 idle (64), and the sizes
# past the streaming kernel's LDS (3080, 4096), which every ln_variant runs on the one-wave kernel.
LN_HS = [8, 64, 256, 512, 520, 768, 1024, 1536, 2048, 2560, 3072, 3080, 4096]
# (B, L, split).  (64, 42, 13): rows_per_wg = 11, the streaming kernel's prefetch loop runs and its last workgroup is short; (2, 42, 13)
# straddles the split and the batch inside a workgroup of the one-wave kernel; (2, 5, 2): odd L (a row pair crosses the batch boundary)
LN_SHAPES = [(1, 1, 0), (1, 1, 1), (1, 7, 3), (3, 9, 4), (2, 42, 13), (2, 5, 2), (64, 42, 13)]
LN_VARIANTS = [1, 2, 3]  # fluxmi_tuning_t.ln_variant: one wave per row | streaming | streaming at two workgroups per CU


def ln_arm(H, variant):
    """the kernel instantiation the launcher picks (csrc/elementwise.hip, LNS / LNM): named in the test ids"""
    nch = next(n for n in (1, 2, 4, 6, 8) if -(-H // 512) <= n)
    if variant >= 2 and H * 16 <= 49152:
        return f"stream-nch{nch}-{'full' if H == nch * 512 else 'guarded'}"
    return f"onewave-nch{nch}"


def _ln_cases():
    """(H, B, L, split, variant, fmt, strided), thinned: every (H, variant, format) once, on a shape that cycles (small H: the large shapes,
    so that one launch fills the pool); every shape at H in {64, 520, 3072} under the one-wave and the streaming kernel (the one-row shapes at
    H = 64, 64 launches each: under one of them).  `strided`: x and
    out are column slices of wider buffers (ldx, ldo > H); it alternates, so every H and every format has dense and strided cases."""
    cases, seen, i = [], set(), 0
    fmts = list(FMTS)

    def put(H, shape, v, f):
        if (H, shape, v, f) not in seen:
            seen.add((H, shape, v, f))
            cases.append((H, *shape, v, f, len(cases) % 2 == 1))

    for H in LN_HS:
        for v in LN_VARIANTS:
            for f in fmts:
                if H <= 64:
                    shape = LN_SHAPES[6]
                else:
                    shape = LN_SHAPES[2 + i % 4]  # (64, 42, 13) at large H only below: its fp64 reference is the slow one
                put(H, shape, v, f)
                i += 1
    for H in (64, 520, 3072):
        for j, shape in enumerate(LN_SHAPES):
            many = reps_for(shape[0] * shape[1] * H) > 8  # a one-row shape at H = 64 fills the pool with 64 launches: one kernel each, bf16
            for v in ((1 + j % 2,) if many else (1, 2)):
                put(H, shape, v, "bf16" if many else fmts[(j + v) % 3])
    return cases


LN_CASES = _ln_cases()


def ln_case_id(c):
    H, B, L, split, v, f, strided = c
    return f"H{H}-B{B}L{L}s{split}-v{v}-{ln_arm(H, v)}-{f}-{'strided' if strided else 'dense'}"


# DC offsets and amplitudes: (H, kind, value) on the shape (2, 42, 13).  An offset r gives every row |mean| / std = r.
LN_OFFSET_SHAPE = (2, 42, 13)
LN_OFFSETS = [(H, "offset", r) for H in (520, 3072) for r in (0, 8, 32, 100)] + [(H, "amp", a) for H in (520, 3072) for a in (1e-3, 1e4)]
# With a DC offset no fp32 kernel reaches min_exact = 0.999: the row mean is known to half an fp32 ulp OF THE OFFSET, which moves
# (x - mean) * rstd across bf16 rounding boundaries.  For these cases min_exact comes from the fp32 models above (ln_modulate_fp32, both
# orders, on this module's seeded inputs, measured on the CPU; tests/test_block_refs_cpu.py repeats the measurement): the lower of the two
# bit-exact shares minus 0.002, floored at 0.99, and never above the 0.999 of the plain cases.  The 2-ulp bound is unchanged.  Measured
# bit-exact shares (one_wave, pairwise) -- the two orders agree to every digit here: the lane sums of 8..48 bf16 values of one magnitude
# are exact in fp32 -- and the worst err / tol of the 2-ulp bound:
#   H = 520:  r = 0: 1.00000 (0.00)   r = 8: 0.99982 (0.42)   r = 32: 0.99895 (0.56)   r = 100: 0.99936 (0.46)
#   H = 3072: r = 0: 0.99999 (0.30)   r = 8: 0.99990 (0.50)   r = 32: 0.99994 (0.43)   r = 100: 0.99864 (0.74)
#   amplitude 1e-3: 0.99995 (0.48) / 0.99999 (0.22); amplitude 1e4: 1.00000 / 1.00000       (H = 520 / 3072)
# Offset 0 and the amplitude cases are plain cases (0.999).
LN_OFFSET_MEASURED = {  # (H, r): (one_wave, pairwise)
    (520, 8): (0.99982, 0.99982), (520, 32): (0.99895, 0.99895), (520, 100): (0.99936, 0.99936),
    (3072, 8): (0.99990, 0.99990), (3072, 32): (0.99994, 0.99994), (3072, 100): (0.99864, 0.99864),
}


def ln_offset_min_exact(H, kind, value):
    if kind != "offset" or value == 0:
        return 0.999
    return min(0.999, max(0.99, min(LN_OFFSET_MEASURED[(H, value)]) - 0.002))


@functools.lru_cache(maxsize=None)
def ln_case_data(H, B, L, split, rep=0, kind=None, value=None):
    """inputs and reference of one launch, computed once and shared: (x, sh0, sc0, sh1, sc1, ref bf16, mag)"""
    kw = {} if kind is None else ({"offset": value} if kind == "offset" else {"amp": value})
    x, sh0, sc0, sh1, sc1 = ln_inputs(B, L, H, seed_of("ln", H, B, L, split, rep, kind, value), **kw)
    ref, mag = ln_modulate_ref(x, sh0, sc0, sh1, sc1, split)
    return x, sh0, sc0, sh1, sc1, ref, mag


# ---- qkv_rope --------------------------------------------------------------------------------------------------------------------
QKV_CASES = [(1, 1, 1, 0), (1, 1, 1, 1), (1, 2, 33, 8), (2, 3, 63, 0), (1, 1, 64, 64), (1, 2, 65, 1), (2, 3, 200, 72), (1, 24, 97, 64),
             (3, 2, 130, 129)]  # (B, H, L, split)
QKV_MODES = {"default": (False, False), "skip_q": (True, False), "skip_q+k_f16": (True, True), "k_f16": (False, True)}  # (skip_q, k_f16)
QKV_LD_EXTRA = [0, 64]  # row stride 3 * H * 128 and 3 * H * 128 + 64


def qkv_inputs(B, H, L, seed, ld_extra=0):
    """qkv [B, L, 3*H*128] bf16 as a view of a [B, L, 3*H*128 + ld_extra] buffer whose extra columns hold the NaN sentinel, pe [B, L, 64, 2]
    (bf16 cos, sin of random angles), and the norm scales (q0, k0, q1, k1) [128]: stream 1's are three times stream 0's."""
    g = torch.Generator().manual_seed(seed)
    full = sentinel_like((B, L, 3 * H * 128 + ld_extra))
    full[..., :3 * H * 128] = torch.randn(B, L, 3 * H * 128, generator=g).bfloat16()
    ang = torch.rand(B, L, 64, generator=g, dtype=torch.float64) * (2 * math.pi)
    pe = torch.stack((torch.cos(ang), torch.sin(ang)), -1).bfloat16()
    s = [((1 + 0.1 * torch.randn(128, generator=g)) * m).bfloat16() for m in (1.0, 1.0, 3.0, 3.0)]
    return full[..., :3 * H * 128], pe, s


def vt_key_order(Lp):
    """storage position -> key: inside every 16-key group bits 2 and 3 of the position are swapped"""
    pos = torch.arange(Lp)
    j = pos % 16
    return (pos // 16) * 16 + ((j & 3) | (((j >> 2) & 1) << 3) | (((j >> 3) & 1) << 2))


def qkv_rope_ref(qkv, pe, s, H, split, mut=None):
    """-> Q, K bf16 [B, H, L, 128], VT bf16 [B, H, 128, Lp] (Lp = L rounded up to 64; columns [L, Lp) zero), the unrounded K, and the
    magnitudes of Q and K for gate_qk: |bf16(c x0)| + |bf16(s x1)|, the terms each rotated value is the rounded sum of"""
    B, L, _ = qkv.shape
    x = qkv.double().view(B, L, 3, H, 128)
    if mut == "heads_swapped" and H > 1:  # heads 2i and 2i + 1 exchanged (an odd last head stays)
        idx = torch.arange(H)
        idx[:H // 2 * 2] = idx[:H // 2 * 2] ^ 1
        x = x[:, :, :, idx]
    l = torch.arange(L)[None, :, None, None]
    st0 = (l <= split) if mut == "stream0_on_first_image_row" else (l < split)
    ped = pe.double()
    if mut == "pe_prev_token":
        ped = torch.roll(ped, 1, 1)
    c, sn = ped[..., 0][:, :, None], ped[..., 1][:, :, None]  # [B, L, 1, 64]
    if mut == "rotation_sign":
        sn = -sn
    outs, mags = [], []
    for part, (w0, w1) in enumerate(((s[0], s[2]), (s[1], s[3]))):
        xp = x[:, :, part]  # [B, L, H, 128]
        rinv = 1.0 / torch.sqrt((xp * xp).mean(-1, keepdim=True) + 1e-6)
        xn = rbf64((xp * rinv) * torch.where(st0, w0.double(), w1.double()))
        x0, x1 = xn[..., 0::2], xn[..., 1::2]
        y0 = rbf64(c * x0) + rbf64(-sn * x1)
        y1 = rbf64(sn * x0) + rbf64(c * x1)
        y = torch.stack((y0, y1), -1).reshape(B, L, H, 128)
        outs.append(y.permute(0, 2, 1, 3).contiguous())  # unrounded sums: exact in fp64
        m = torch.stack((rbf64(c * x0).abs() + rbf64(sn * x1).abs(), rbf64(sn * x0).abs() + rbf64(c * x1).abs()), -1)
        mags.append(m.reshape(B, L, H, 128).permute(0, 2, 1, 3).contiguous())
    Lp = (L + 63) // 64 * 64
    vpad = torch.zeros(B, H, Lp, 128, dtype=torch.bfloat16)
    vpad[:, :, :L] = x[:, :, 2].permute(0, 2, 1, 3).bfloat16()
    key = torch.arange(Lp) if mut == "vt_unpermuted" else vt_key_order(Lp)
    VT = vpad[:, :, key].transpose(-1, -2).contiguous()
    return round_fp64_to_bf16(outs[0]), round_fp64_to_bf16(outs[1]), VT, outs[1], mags[0], mags[1]


def k_as_f16(K_bf16, k_unrounded=None, mut=None):
    """the fp16 form of K: fp16 of the bf16 VALUE (exact unless |k| < 2^-14).  mut: fp16 straight from the unrounded sum."""
    if mut == "f16_from_unrounded":
        return k_unrounded.to(torch.float16)
    return K_bf16.float().to(torch.float16)


def qkv_rope_fp32(qkv, pe, s, H, split):
    """the kernel's arithmetic in torch fp32: sum of squares per lane of 8 then the 16-lane xor butterfly, rinv = 1 / sqrt(ss / 128 + 1e-6)"""
    B, L, _ = qkv.shape
    x = qkv.float().view(B, L, 3, H, 128)
    st0 = torch.arange(L)[None, :, None, None] < split
    c, sn = pe.float()[..., 0][:, :, None], pe.float()[..., 1][:, :, None]
    outs = []
    for part, (w0, w1) in enumerate(((s[0], s[2]), (s[1], s[3]))):
        xp = x[:, :, part]
        sq = (xp * xp).view(B, L, H, 16, 8)
        ss = torch.zeros(B, L, H, 16)
        for j in range(8):
            ss = ss + sq[..., j]
        lane = torch.arange(16)
        for o in (8, 4, 2, 1):
            ss = ss + ss[..., lane ^ o]
        rinv = 1.0 / torch.sqrt(ss[..., :1] * (1.0 / 128.0) + 1e-6)
        xn = _r32((xp * rinv) * torch.where(st0, w0.float(), w1.float()))
        x0, x1 = xn[..., 0::2], xn[..., 1::2]
        y0 = _r32(_r32(c * x0) + _r32(-sn * x1))
        y1 = _r32(_r32(sn * x0) + _r32(c * x1))
        outs.append(torch.stack((y0, y1), -1).reshape(B, L, H, 128).permute(0, 2, 1, 3).bfloat16().contiguous())
    return outs[0], outs[1]


def gate_qk(got, ref, mag, what):
    """test_qkv_rope's gate -- at most 1 bf16 ulp from the reference, 0.999 identical -- with one allowance: a value further than 1 ulp
    passes if it is within one bf16 ulp AT `mag` (assert_close_mag's measure; mag from qkv_rope_ref).  The rotation subtracts: where
    bf16(c x0) and bf16(s x1) cancel, a 1-ulp flip of the normalised x (any fp32 rinv is off by 6e-8, which moves 2e-5 of the values
    across a bf16 rounding boundary) is more than 1 ulp of the small difference.  qkv_rope_fp32 does that at 3 of the 9 cases (1 to 3 values
    of 1e5, 2 ulps): the plain bound is not attainable in fp32 at these sizes.  The 0.999 share is taken over all values, unchanged."""
    g, r = got.detach().cpu(), ref.detach().cpu()
    d = (bf16_ord(g) - bf16_ord(r)).abs()
    exact = (d == 0).float().mean().item()
    far = (d > 1) & ((g.double() - r.double()).abs() > torch.maximum(r.double().abs(), mag.reshape(r.shape)) * 2.0 ** -7)
    assert not bool(far.any()) and exact >= 0.999, (
        f"{what}: {int(far.sum())} values beyond 1 bf16 ulp and beyond 1 ulp at the rotation's magnitude (max ulp diff {int(d.max())}), "
        f"exact fraction {exact:.5f} (need 0.999)")
    return exact


def gate_k_f16(got16, ref_bf16, mag, what):
    """fp16 K: every value is the fp16 of a bf16 value (on the bf16 grid; below fp16's normal range, 2^-14, the grid is fp16's own), and
    those bf16 values pass the Q / K gate"""
    g = got16.detach().cpu()
    assert g.dtype == torch.float16, f"{what}: K is {g.dtype}, not float16"
    on_grid = (g.float().bfloat16().float() == g.float()) | (g.float().abs() < 2.0 ** -14)
    assert bool(on_grid.all()), f"{what}: {int((~on_grid).sum())} fp16 values of K are not bf16 values (K was not rounded to bf16 first)"
    big = ref_bf16.float().abs() >= 2.0 ** -14
    return gate_qk(g.float().bfloat16()[big], ref_bf16[big], mag.reshape(ref_bf16.shape)[big], what)


def gate_vt(got, ref, what):
    assert torch.equal(bits(got.cpu()), bits(ref)), f"{what}: V^T differs from the permuted, zero-padded transpose"


@functools.lru_cache(maxsize=None)
def qkv_case_data(B, H, L, split, ld_extra, rep=0):
    qkv, pe, s = qkv_inputs(B, H, L, seed_of("qkv", B, H, L, split, rep), ld_extra)
    Q, K, VT, _, mq, mk = qkv_rope_ref(qkv, pe, s, H, split)
    return qkv, pe, s, Q, K, VT, mq, mk


# ---- the exact chains ------------------------------------------------------------------------------------------------------------
def gate_residual_ref(x, y, gate):
    """x, y [B, L, H], gate [B, H]: bf16(x + bf16(gate * y)); the product of two bf16 values is exact in fp32 and in fp64"""
    return round_fp64_to_bf16(x.double() + rbf64(gate.double()[:, None] * y.double()))


def add_ref(a, b):
    return round_fp64_to_bf16(a.double() + b.double())


def add_bcast_ref(a, b):
    """a [rows, cols], b [nb, cols]: row r takes b[r % nb]"""
    return round_fp64_to_bf16(a.double() + b.double()[torch.arange(a.shape[0]) % b.shape[0]])


def euler_ref(img, pred, dt):
    """bf16(img + bf16(dt * pred)): dt is an fp32 value, and the kernel forms dt * pred in fp32 (24 x 8 significant bits: it rounds) before
    the bf16 rounding -- both roundings are the operation's"""
    dt32 = torch.tensor(dt, dtype=torch.float32).double()
    p = (dt32 * pred.double()).float().bfloat16()
    return round_fp64_to_bf16(img.double() + p.double())


def pair_rows_ref(w):
    """[R, C] -> the same bytes as [R/2][row_bytes/64][2][64] (fluxmi_pair_rows), as a tensor of w's shape"""
    R = w.shape[0]
    b = w.contiguous().view(torch.uint8).view(R // 2, 2, -1, 64)
    return b.permute(0, 2, 1, 3).contiguous().view(R, -1).view(w.dtype).view(w.shape)


# ---- tables ----------------------------------------------------------------------------------------------------------------------
ROPE_POSITIONS = list(range(17)) + [63, 64, 127, 255, 511, 1023]
AXES_DIM, THETA = [16, 56, 56], 10000


def rope_ids():
    """ids [1, rows, 3] bf16: every position on each axis alone (the others 0) and on all three at once"""
    rows = []
    for p in ROPE_POSITIONS:
        rows += [[p, 0, 0], [0, p, 0], [0, 0, p], [p, p, p]]
    return torch.tensor(rows, dtype=torch.float32).bfloat16()[None]


def rope_omega():
    """the host constants of ops.rope_tables_host (flux_model.py:50-51)"""
    om, ax = [], []
    for i, d in enumerate(AXES_DIM):
        o = 1.0 / (THETA ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
        om.append(o)
        ax += [i] * o.numel()
    return torch.cat(om), torch.tensor(ax)


def rope_table_ref(ids, fp32=False):
    """-> [B, L, 64, 2] bf16 (cos, sin) of the fp32 product float(ids) * omega; fp32 = True: torch's fp32 cos / sin (the fp32 model)"""
    om, ax = rope_omega()
    ang = ids.float()[..., ax] * om  # fp32 product, as the kernel forms it
    if fp32:
        return torch.stack((torch.cos(ang), torch.sin(ang)), -1).bfloat16()
    return round_fp64_to_bf16(torch.stack((torch.cos(ang.double()), torch.sin(ang.double())), -1))


def timestep_values():
    """every bf16 t in [0, 1] (bit patterns 0x0000 .. 0x3F80) and the guidance values"""
    t = torch.arange(0, 0x3F80 + 1, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    return torch.cat((t, torch.tensor([1.0, 3.5, 10.0, 30.0]).bfloat16()))


def timestep_freqs(half=128, max_period=10000):
    return torch.exp(-math.log(max_period) * torch.arange(0, half, dtype=torch.float32) / half)


def timestep_embedding_ref(t, fp32=False, time_factor=1000.0):
    """-> [B, 256] bf16: cos | sin of the fp32 product bf16(1000 t) * freq"""
    tt = round_fp64_to_bf16(time_factor * t.double()).float()
    arg = tt[:, None] * timestep_freqs()[None]
    if fp32:
        return torch.cat((torch.cos(arg), torch.sin(arg)), -1).bfloat16()
    return round_fp64_to_bf16(torch.cat((torch.cos(arg.double()), torch.sin(arg.double())), -1))


def gate_rope(got, ref, what):
    return assert_bf16_close(got, ref, max_ulp=1, min_exact=0.999, what=what)


def gate_timestep(got, ref, what):
    return assert_bf16_close(got, ref, max_ulp=1, min_exact=0.995, what=what)


def max_ulp(got, ref):
    return int((bf16_ord(got.cpu()) - bf16_ord(ref.cpu())).abs().max())
