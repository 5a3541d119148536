"""The helper kernels around the GEMM and the flow attention -- gemv, the VAE's groupnorm and softmax_rows, the encoders' row_norm, act_mul
and text / vision attention -- against fp64 references (tests/helper_refs.py) at ragged sizes, strided views and poisoned padding.

The gates are the ones the first tests of these kernels set (tests/test_ops_gpu.py); tests/test_helper_refs_cpu.py shows that each rejects
the wrong kernels it is meant to catch and that torch's fp32 kernels pass it.  Every buffer a kernel must not write (stride gaps, rows >= L,
columns >= N) is filled with a bf16 sentinel before the call and compared bit for bit afterwards.  Each test prints its worst figure.
"""
import pytest
import torch

import helper_refs as hr
from helper_refs import bits, sentinel_like
from parity_util import accum_noise, assert_close_mag, bf16_ord, round_fp64_to_bf16

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(dev):
    from fluxmi import ops as _ops

    return _ops


def assert_sentinel(t, what):
    assert bool((bits(t.cpu()) == bits(sentinel_like((1,)))).all()), f"{what}: a sentinel was overwritten"


def worst_ratio(got, ref, mag, ulps=1.0):
    g, r = got.detach().cpu().double(), ref.detach().cpu().double()
    m = mag.detach().cpu().double() if torch.is_tensor(mag) else torch.full_like(r, float(mag))
    return float(((g - r).abs() / (ulps * torch.maximum(r.abs(), m) * 2.0 ** -7).clamp_min(1e-300)).max())


# ---- gemv ----------------------------------------------------------------------------------------------------------------------
def run_gemv(ops, dev, K, N, B, mode, opts, seed):
    """one launch; returns (got [B, N] on the host, fp64 reference, accumulation noise)"""
    w_fp8, fmt, pre_silu = hr.GEMV_MODES[mode]
    x, w, bias = hr.gemv_inputs(B, K, N, seed)
    if "nobias" in opts:
        bias = None
    a, w_op, s, extras = hr.gemv_operands(x, w, w_fp8, fmt, pre_silu)
    ref = hr.gemv_ref(a, w_op, s, bias)
    xd = x.to(dev)
    if "xview" in opts:  # a column slice of a wider buffer: ldx = K + 64
        xbuf = sentinel_like((B, K + 64), dev)
        xbuf[:, 32:32 + K] = xd
        xd = xbuf[:, 32:32 + K]
    obuf = sentinel_like((B, N + 48) if "outview" in opts else (B, N), dev)
    out = obuf[:, 24:24 + N] if "outview" in opts else obuf
    sc = [None, None, None] if extras is None else [t.to(dev) for t in extras]
    ops.gemv(xd, w_op.to(dev), None if bias is None else bias.to(dev), sc[0], sc[1], sc[2], pre_silu=pre_silu, act_fmt=fmt, out=out)
    torch.cuda.synchronize()
    if "outview" in opts:
        assert_sentinel(obuf[:, :24], "gemv out, columns before the view")
        assert_sentinel(obuf[:, 24 + N:], "gemv out, columns past N")
    return out.cpu(), ref, accum_noise(a, w_op, s)


def test_gemv_96k_lds_first_call_and_after_a_small_one(ops, dev):
    """B = 8, K = 3072 needs 96 KB of LDS, past the 64 KB a kernel gets without the dynamic-LDS attribute.  Defined first: run on its own it
    is this process's first gemv launch; after a K = 256 launch the same call must give the same bits.  (The launcher remembers in one
    process-wide variable that it raised the attribute; on one device that is right in either order, which is all this test can show -- a
    process that drives several devices would need it per device.)"""
    case = (3072, 200, 8, "fp8_e5m2_silu", "", 1)
    got0, ref, noise = run_gemv(ops, dev, *case)
    ex = hr.gate_gemv(got0, ref, noise, "gemv B=8 K=3072, first call")
    run_gemv(ops, dev, 256, 64, 1, "bf16", "", 2)
    got1, _, _ = run_gemv(ops, dev, *case)
    assert torch.equal(bits(got0), bits(got1)), "gemv B=8 K=3072 differs after a K=256 call"
    print(f"gemv 96 KB LDS: worst err/tol {worst_ratio(got0, round_fp64_to_bf16(ref), noise):.3f} (<= 1), bit-exact {ex:.4f} (>= 0.98)")


@pytest.mark.parametrize("K,N,B,mode,opts", hr.GEMV_CASES, ids=lambda v: str(v).replace(" ", "+") or "plain")
def test_gemv(ops, dev, K, N, B, mode, opts):
    gots, refs, noises = [], [], []
    for rep in range(hr.gemv_reps(B, N)):  # small outputs: fresh seeds, gated together (min_exact needs a population)
        g, r, n = run_gemv(ops, dev, K, N, B, mode, opts, hr.seed_of("gemv", K, N, B, mode, rep))
        gots.append(g), refs.append(r), noises.append(n)
    got, ref, noise = torch.cat(gots), torch.cat(refs), torch.cat(noises)
    ex = hr.gate_gemv(got, ref, noise, f"gemv K={K} N={N} B={B} {mode} {opts}")
    print(f"gemv K={K} N={N} B={B} {mode} [{opts}]: worst err/tol {worst_ratio(got, round_fp64_to_bf16(ref), noise):.3f} (<= 1), "
          f"bit-exact {ex:.4f} (>= 0.98) over {got.numel()} values")


def test_gemv_refuses_what_does_not_fit_in_lds(ops, dev):
    B, K, N = 8, 5136, 64  # 8 * 5136 * 4 = 164352 bytes > 160 KB
    x = torch.randn(B, K, generator=torch.Generator().manual_seed(3)).bfloat16().to(dev)
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(4)).bfloat16().to(dev)
    out = sentinel_like((B, N), dev)
    with pytest.raises(RuntimeError, match="too large for LDS"):
        ops.gemv(x, w, out=out)
    torch.cuda.synchronize()
    assert_sentinel(out, "gemv out after the refusal")


# ---- groupnorm -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,P,swish", hr.GROUPNORM_CASES)
def test_groupnorm(ops, dev, C, P, swish):
    x, ga, be = hr.groupnorm_inputs(3, P, C, hr.seed_of("gn", C, P, swish))
    ref = hr.groupnorm_ref(x, ga, be, swish)
    got = ops.groupnorm(x.to(dev), ga.to(dev), be.to(dev), swish=swish).cpu()
    print(f"groupnorm C={C} P={P} swish={swish}: worst err/tol {worst_ratio(got, ref, 0.25):.3f} (<= 1), "
          f"bit-exact {(got == ref).double().mean().item():.4f} (>= 0.99)")
    hr.gate_groupnorm(got, ref, f"groupnorm C={C} P={P} swish={swish}")
    # the statistics of an image are its own: other data in batch 1 changes nothing in batches 0 and 2
    x2 = x.clone()
    x2[1] = hr.groupnorm_inputs(1, P, C, 12345)[0][0] * 3 + 7
    got2 = ops.groupnorm(x2.to(dev), ga.to(dev), be.to(dev), swish=swish).cpu()
    assert torch.equal(bits(got2[0]), bits(got[0])) and torch.equal(bits(got2[2]), bits(got[2])), "groupnorm: batch b depends on another batch"
    hr.gate_groupnorm(got2[1:2], hr.groupnorm_ref(x2[1:2], ga, be, swish), f"groupnorm C={C} P={P}: the replaced batch")


@pytest.mark.parametrize("swish", [True, False])
@pytest.mark.parametrize("r", hr.GROUPNORM_OFFSETS)
def test_groupnorm_dc_offsets(ops, dev, r, swish):
    """VAE activations carry DC offsets: groups with |mean| / std = r (std 1, another mean per group).  The kernel must pass the gate that
    torch's fp32 group_norm passes on these inputs (tests/test_helper_refs_cpu.py).  gn_partial sums x and x^2 about zero in fp32, and the
    cancellation in E[x^2] - E[x]^2 shows: measured bit-exact shares 1.0000 / 0.9996 / 0.9967 / 0.9921 at r = 0 / 8 / 32 / 64 (need 0.99),
    no element beyond one ulp.  It passes at 64, with little room: this test is the guard for wider offsets or longer fp32 chains."""
    x, ga, be = hr.groupnorm_inputs(3, 1025, 128, hr.seed_of("gn-offset", r), offsets=r)
    ref = hr.groupnorm_ref(x, ga, be, swish)
    got = ops.groupnorm(x.to(dev), ga.to(dev), be.to(dev), swish=swish).cpu()
    print(f"groupnorm offsets mean/std={r} swish={swish}: worst err/tol {worst_ratio(got, ref, 0.25):.3f} (<= 1), "
          f"bit-exact {(got == ref).double().mean().item():.4f} (>= 0.99)")
    hr.gate_groupnorm(got, ref, f"groupnorm mean/std={r} swish={swish}")


# ---- softmax_rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", hr.SOFTMAX_SCALES)
@pytest.mark.parametrize("cols", hr.SOFTMAX_COLS)
def test_softmax_rows(ops, dev, cols, scale):
    from fluxmi import _lib

    S = hr.softmax_inputs(cols, hr.seed_of("softmax", cols))
    ref = hr.softmax_ref(S, scale)
    got = ops.softmax_rows(S.to(dev), scale).cpu()
    d = (bf16_ord(got) - bf16_ord(ref)).abs()
    print(f"softmax_rows cols={cols} scale={scale}: max ulp {int(d.max())} (<= 1), bit-exact {(d == 0).double().mean().item():.4f} (>= 0.99)")
    hr.gate_softmax(got, ref, f"softmax_rows cols={cols} scale={scale}")
    assert got[4, cols // 3] == 0, "the -inf entry's probability is exactly 0"
    # ld = cols + 64 on the input view and the output (one ld for both in the C ABI), sentinels in the gap
    ld = cols + 64
    sbuf, pbuf = sentinel_like((5, ld), dev), sentinel_like((5, ld), dev)
    sbuf[:, :cols] = S.to(dev)
    _lib.call("fluxmi_softmax_rows", ops._p(sbuf), ops._p(pbuf), 5, cols, ld, float(scale), ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(bits(pbuf[:, :cols].cpu()), bits(got)), "softmax_rows: ld > cols changes the result"
    assert_sentinel(pbuf[:, cols:], "softmax_rows out, columns >= cols")
    assert_sentinel(sbuf[:, cols:], "softmax_rows in, columns >= cols")


# ---- row_norm ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rms,kind", hr.ROW_NORM_KINDS)
@pytest.mark.parametrize("D", hr.ROW_NORM_DS)
def test_row_norm(ops, dev, D, rms, kind):
    from fluxmi import _lib

    x, w, b = hr.row_norm_inputs(D, rms, kind, hr.seed_of("row_norm", D, kind))
    eps = 1e-6 if rms else 1e-5
    ref = hr.row_norm_ref(x, w, b, eps, rms)
    wd, bd = w.to(dev), None if rms else b.to(dev)
    got = ops.row_norm(x.to(dev), wd, bd, eps=eps, rms=rms).cpu()
    d = (bf16_ord(got) - bf16_ord(ref)).abs()
    print(f"row_norm D={D} rms={rms} {kind}: max ulp {int(d.max())} (<= 1), bit-exact {(d == 0).double().mean().item():.4f} (>= 0.98)")
    hr.gate_row_norm(got, ref, f"row_norm D={D} rms={rms} {kind}")
    # x as a view with ldx = D + 8 (through the wrapper), then ldy = D + 8 as well (through the C ABI), sentinels in both gaps
    xbuf = sentinel_like((5, D + 8), dev)
    xbuf[:, :D] = x.to(dev)
    got_v = ops.row_norm(xbuf[:, :D], wd, bd, eps=eps, rms=rms).cpu()
    assert torch.equal(bits(got_v), bits(got)), "row_norm: ldx > D changes the result"
    ybuf = sentinel_like((5, D + 8), dev)
    _lib.call("fluxmi_row_norm", ops._p(xbuf), ops._p(wd), None if rms else ops._p(bd), ops._p(ybuf), 5, D, D + 8, D + 8, float(eps),
              0 if rms else 1, ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(bits(ybuf[:, :D].cpu()), bits(got)), "row_norm: ldy > D changes the result"
    assert_sentinel(ybuf[:, D:], "row_norm out, columns >= D")
    assert_sentinel(xbuf[:, D:], "row_norm in, columns >= D")


# ---- act_mul -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b_kind", [None, 1.0, -3.5, "random"], ids=["quick_gelu", "b=1", "b=-3.5", "b=random"])
def test_act_mul_every_finite_bf16(ops, dev, b_kind):
    x, a, b = hr.act_sweep_inputs(b_kind)  # [8160, 8] or [8160, 16]: F = 8, and 8160 is no multiple of the 256-thread blocks
    ref = hr.act_mul_ref(a, b)
    got = ops.act_mul(x.to(dev), gated=b_kind is not None).cpu()
    fin = torch.isfinite(ref.float())
    mag = 1e-4 if b is None else (1e-4 * b.double().abs())[fin]
    print(f"act_mul {b_kind}: worst err/tol {worst_ratio(got[fin], ref[fin], mag):.3f} (<= 1), "
          f"bit-exact {(got[fin] == ref[fin]).double().mean().item():.5f} (>= 0.999), left out as non-finite {1 - fin.double().mean().item():.5f}")
    if b_kind == 1.0:  # for the record: against gelu_new WITHOUT the documented fp32 rounding of tanh (measured 0.99763: the cancelling tail)
        exact = round_fp64_to_bf16(hr.gelu_new_exact64(a.double()))
        print(f"act_mul b=1 vs the unrounded fp64 gelu_new: bit-exact {(got == exact).double().mean().item():.5f} (not gated)")
    left_out = hr.gate_act(got, ref, b, f"act_mul {b_kind}")
    assert left_out < 0.01


@pytest.mark.parametrize("gated", [True, False])
def test_act_mul_strided(ops, dev, gated):
    from fluxmi import _lib

    R, F_ = 37, 8
    g = torch.Generator().manual_seed(21)
    x = (torch.randn(R, 2 * F_ if gated else F_, generator=g) * 2).bfloat16()
    ref = hr.act_mul_ref(x[:, :F_], x[:, F_:] if gated else None)
    ld_in, ld_out = 2 * F_ + 16, F_ + 8
    ibuf, obuf = sentinel_like((R, ld_in), dev), sentinel_like((R, ld_out), dev)
    ibuf[:, : x.shape[1]] = x.to(dev)
    _lib.call("fluxmi_act_mul", ops._p(ibuf), ops._p(obuf), R, F_, ld_in, ld_out, 0 if gated else 1, ops._stream())
    torch.cuda.synchronize()
    got = obuf[:, :F_].cpu()
    assert torch.equal(bits(got), bits(ops.act_mul(x.to(dev), gated=gated).cpu())), "act_mul: strides change the result"
    # 296 values are no population for a bit-exact share: the per-element half of the gate only (the sweep above carries the rest)
    assert_close_mag(got, ref, mag=1e-4 * x[:, F_:].double().abs() if gated else 1e-4, ulps=1, min_exact=0.0, what=f"act_mul strided gated={gated}")
    assert_sentinel(obuf[:, F_:], "act_mul out, columns >= F")
    assert_sentinel(ibuf[:, x.shape[1]:], "act_mul in, columns past the row")


# ---- text / vision attention ---------------------------------------------------------------------------------------------------
def run_attention(ops, dev, q, k, v, L, H, D, scale, causal, rel, vb, batched):
    """q, k, v [B, Lp, H*D] on the host (padding rows as given).  V^T gets ld_vt = Lp + 32 (its padding columns continue v's padding rows'
    pattern), out is a column view of a sentinel-filled [.., H*D + 64] buffer.  Returns (out rows < L as [B, L, H*D], the out buffer)."""
    B, Lp = q.shape[0], q.shape[1]
    ld = 2 * H * D
    qk = torch.zeros(B, Lp + 2, ld, dtype=torch.bfloat16)  # two rows more per image: a batch stride above the minimum
    qk[:, :Lp, : H * D], qk[:, :Lp, H * D:] = q, k
    qk[:, Lp:] = qk[:, Lp - 1:Lp] if L < Lp else 0
    vt = torch.zeros(B, H * D + 4, Lp + 32, dtype=torch.bfloat16)
    vt[:, : H * D, :Lp] = v.transpose(1, 2)
    if L < Lp:
        vt[:, :, Lp:] = vt[:, :, Lp - 1:Lp]  # poisoned runs: the columns up to ld_vt are poisoned too
    qk, vt = qk.to(dev), vt.to(dev)
    obuf = sentinel_like((B, Lp + 1, H * D + 64), dev)
    out = obuf[:, :Lp, 32:32 + H * D]
    kw = dict(v_bias=None if vb is None else vb.to(dev))
    if batched:
        ops.vision_attention(qk[:, :Lp, : H * D], qk[:, :Lp, H * D:], vt[:, : H * D, :Lp], L, H, D, scale, out=out, **kw)
    else:
        assert B == 1 and D == 64
        ops.text_attention(qk[0, :Lp, : H * D], qk[0, :Lp, H * D:], vt[0, : H * D, :Lp], L, H, scale=scale, causal=causal,
                           rel_bias=None if rel is None else rel.to(dev), out=out[0], **kw)
    torch.cuda.synchronize()
    return out[:, :L].cpu(), obuf.cpu()


def check_attention(ops, dev, L, H, D, style, bias_extra, B, batched, what):
    q, k, v, rel, vb, scale, causal = hr.attention_inputs(L, H, D, style, hr.seed_of("attn", L, H, D, style, bias_extra), B=B, bias_extra=bias_extra)
    Lp = q.shape[1]
    got, obuf = run_attention(ops, dev, q, k, v, L, H, D, scale, causal, rel, vb, batched)
    worst = 0.0
    for b in range(B):
        ref = hr.attention_ref(q[b], k[b], v[b], L, H, D, scale, causal, rel, vb)
        ok, w = hr.attention_gate(got[b], ref)
        worst = max(worst, w)
        assert ok, f"{what}: worst err/tol {w:.2f} in sequence {b}"
    print(f"{what}: worst err/tol {worst:.3f} (<= 1)")
    # rows >= L, the columns on both sides of the view and the row past Lp keep the sentinel
    assert_sentinel(obuf[:, L:], f"{what}: out rows >= L")
    assert_sentinel(obuf[:, :, :32], f"{what}: out columns before the view")
    assert_sentinel(obuf[:, :, 32 + H * D:], f"{what}: out columns past H*D")
    # padding must not matter: rows >= L of q and k and columns >= L of V^T (up to ld_vt) at +-1.0e4 -> the same bits
    got_p, obuf_p = run_attention(ops, dev, hr.poison(q, L, 1), hr.poison(k, L, 1), hr.poison(v, L, 1), L, H, D, scale, causal, rel, vb, batched)
    assert torch.equal(bits(got_p), bits(got)), f"{what}: the output depends on the padding"
    assert torch.equal(bits(obuf_p), bits(obuf))


@pytest.mark.parametrize("style,bias_extra", hr.ATTN_STYLES, ids=["t5", "t5_wide_bias", "clip"])
@pytest.mark.parametrize("H", hr.ATTN_HS)
@pytest.mark.parametrize("L", hr.ATTN_LS)
def test_text_attention(ops, dev, L, H, style, bias_extra):
    """L = 1 and 31: lanes whose 16 keys are all masked keep the sentinel maximum until the two halves merge; 33: one key in the second tile;
    1024 = Lp: no padding at all (the poisoned run then equals the first)."""
    check_attention(ops, dev, L, H, 64, style, bias_extra, 1, False, f"text_attention L={L} H={H} {style} bias_ld=2Lp+{bias_extra}")


def test_vision_attention_head_width_96(ops, dev):
    check_attention(ops, dev, 37, 2, 96, "vision", 0, 2, True, "vision_attention D=96 B=2 L=37 H=2")
