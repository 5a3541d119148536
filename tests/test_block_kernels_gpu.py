"""The glue kernels of a transformer block -- ln_modulate, qkv_rope, gate_residual, add / add_bcast, act, euler_, pair_rows / unpair_rows,
rope_table, timestep_embedding (csrc/elementwise.hip, csrc/qkv_rope.hip) -- against the fp64 references of tests/block_refs.py, at every
dispatch arm of the launchers, strided views, ragged sizes and the row-pair layout.

tests/test_block_refs_cpu.py shows that each gate accepts an fp32 model of the kernel and rejects the wrong kernels it is meant to catch.
Every buffer a kernel must not write (stride gaps, rows >= B * L, guard bands around Q / K / V^T) is filled with a bf16 sentinel before the
call and compared bit for bit afterwards.  Small cases are repeated with fresh seeds and gated together (>= 4096 values).  Each test prints
its worst figure.
"""
import pytest
import torch

import block_refs as br
from block_refs import E4M3, E5M2, bits, sentinel_like
from parity_util import f8_ulp_diff

pytestmark = pytest.mark.gpu
GUARD = 256  # elements of sentinel before and after a flat output


@pytest.fixture(scope="module")
def ops(dev):
    from fluxmi import ops as _ops

    return _ops


def u8(t):
    return t.contiguous().view(torch.uint8) if t.is_contiguous() else t.view(torch.uint8)


def sentinel_bytes(rows, row_bytes, dev):
    """[rows, row_bytes] uint8 holding the bf16 sentinel pattern"""
    return sentinel_like((rows, row_bytes // 2), dev).view(torch.uint8)


def assert_only_written(buf, before, region, what):
    """buf, before: uint8 tensors of one shape; region(t) -> the view of t the kernel may write.  Everything else must be unchanged."""
    a, b = buf.clone(), before.clone()
    region(a).zero_()
    region(b).zero_()
    assert torch.equal(a, b), f"{what}: bytes outside the output were written"


def guarded(shape, dtype, dev):
    """a contiguous tensor of `shape` inside a flat sentinel buffer with GUARD elements on either side -> (tensor, flat buffer as int16)"""
    n = 1
    for d in shape:
        n *= d
    flat = sentinel_like((n + 2 * GUARD,), dev)
    return flat[GUARD:GUARD + n].view(dtype).view(shape), flat.view(torch.int16)


def assert_guards(flat, n, what):
    s = bits(sentinel_like((1,))).item()
    assert bool((flat[:GUARD] == s).all()) and bool((flat[GUARD + n:] == s).all()), f"{what}: a guard band was written"


def assert_sentinel(t, what):
    assert bool((bits(t.cpu()) == bits(sentinel_like((1,)))).all()), f"{what}: a sentinel was overwritten"


def worst_ratio(got, ref, mag, ulps):
    g, r = got.detach().cpu().double(), ref.detach().cpu().double()
    return float(((g - r).abs() / (ulps * torch.maximum(r.abs(), mag.double().reshape(r.shape)) * 2.0 ** -7).clamp_min(1e-300)).max())


# ---- ln_modulate ---------------------------------------------------------------------------------------------------------------
def run_ln(ops, dev, data, split, variant, fmt, strided=False, x=None):
    """one launch under ln_variant = variant -> the [B, L, H] output on the host.  strided: x and out are column slices of sentinel-filled
    wider buffers with three spare rows; the gaps and the spare rows must come back untouched."""
    from fluxmi import _lib

    x0, sh0, sc0, sh1, sc1 = data[:5]
    x = x0 if x is None else x
    B, L, H = x.shape
    mods = torch.cat((sh0, sc0, sh1, sc1), 1).to(dev)  # one [B, 4H] table: the vectors keep their row stride of 4H
    v = [mods[:, i * H:(i + 1) * H] for i in range(4)]
    esz = 2 if fmt is None else 1
    odt = torch.bfloat16 if fmt is None else br.F8T[fmt]
    xoff, xw, ooff, ow = (8, H + 24, 16, H + 32) if strided else (0, H, 0, H)
    xbuf = sentinel_like((B * L + 3, xw), dev)
    xv = xbuf[:B * L].view(B, L, xw)[:, :, xoff:xoff + H]
    xv.copy_(x.to(dev))
    obuf = sentinel_bytes(B * L + 3, ow * esz, dev)
    before = obuf.clone()
    ov = obuf.view(odt)[:B * L].view(B, L, ow)[:, :, ooff:ooff + H]
    q = [None, None] if fmt is None else [torch.tensor(s, device=dev) for s in br.LN_QSCALES[fmt]]
    with _lib.tuning(ln_variant=variant):
        ops.ln_modulate(xv, v[0], v[1], v[2], v[3], split=split, q_scale0=q[0], q_scale1=q[1], fmt=E5M2 if fmt is None else fmt, out=ov)
    torch.cuda.synchronize()
    assert_only_written(obuf, before, lambda t: t[:B * L].view(B, L, ow * esz)[:, :, ooff * esz:(ooff + H) * esz], "ln_modulate out")
    return ov.cpu().contiguous()


@pytest.mark.parametrize("case", br.LN_CASES, ids=br.ln_case_id)
def test_ln_modulate(ops, dev, case):
    """Every arm of fluxmi_k_ln_modulate (the id names it).  The bf16 output against the fp64 reference; an fp8 case also requires the fp8
    output to be the quantised bf16 output of the same kernel byte for byte, and gates it against the quantised reference.  The two streaming
    grids (ln_variant 2 and 3) must give the same bits (tests/knob_contract.py), and at H > 3072 all three variants run one kernel.
    Measured on an MI355X over the 149 cases: worst err / tol 0.78, lowest bit-exact share 0.99981; fp8 identical share >= 0.99981, and
    one value 8 fp8 codes off where (1 + scale) LN and shift cancel (|y| < mag / 8: block_refs.gate_ln_f8)."""
    H, B, L, split, variant, fname, strided = case
    fmt = br.FMTS[fname]
    gots, refs, mags, gq, rq = [], [], [], [], []
    for rep in range(br.reps_for(B * L * H)):
        data = br.ln_case_data(H, B, L, split, rep)
        ref, mag = data[5], data[6]
        got = run_ln(ops, dev, data, split, variant, None, strided)
        gots.append(got.reshape(-1)), refs.append(ref.reshape(-1)), mags.append(mag.reshape(-1))
        if fmt is not None:
            got8 = run_ln(ops, dev, data, split, variant, fmt, strided)
            own = br.ln_quant_ref(got, split, *br.LN_QSCALES[fmt], fmt)
            assert torch.equal(u8(got8), u8(own)), f"ln_modulate {fname}: the fp8 output is not quantise(own bf16 output)"
            gq.append(got8.reshape(-1)), rq.append(br.ln_quant_ref(ref, split, *br.LN_QSCALES[fmt], fmt).reshape(-1))
        if rep == 0:
            same = {2: (3,), 3: (2,)}.get(variant, ()) if H * 16 <= 49152 else tuple(v for v in br.LN_VARIANTS if v != variant)
            for other in same:
                o = run_ln(ops, dev, data, split, other, fmt, strided)
                assert torch.equal(u8(o), u8(got if fmt is None else got8)), f"ln_modulate H={H}: ln_variant {other} and {variant} differ"
    got, ref, mag = torch.cat(gots), torch.cat(refs), torch.cat(mags)
    line = f"ln_modulate {br.ln_case_id(case)}: worst err/tol {worst_ratio(got, ref, mag, 2):.3f} (<= 1), bit-exact {(got == ref).double().mean().item():.5f} (>= 0.999)"
    if fmt is not None:
        d = f8_ulp_diff(torch.cat(gq), torch.cat(rq))
        line += f"; fp8 max code diff {int(d.max())}, identical {(d == 0).double().mean().item():.5f} (>= 0.999)"
    print(line + f" over {got.numel()} values")
    br.gate_ln_bf16(got, ref, mag, f"ln_modulate bf16 {br.ln_case_id(case)}")
    if fmt is not None:
        br.gate_ln_f8(torch.cat(gq), torch.cat(rq), f"ln_modulate {br.ln_case_id(case)}", y=ref, mag=mag)


@pytest.mark.parametrize("variant", br.LN_VARIANTS)
@pytest.mark.parametrize("H,kind,value", br.LN_OFFSETS)
def test_ln_modulate_dc_offsets_and_amplitudes(ops, dev, H, kind, value, variant):
    """Rows with |mean| / std up to 100, and amplitudes at which eps dominates the variance (1e-3) or vanishes (1e4).  The 2-ulp bound is
    the plain one; the bit-exact share required under an offset is what the fp32 models of tests/block_refs.py reach on these inputs,
    less 0.002 (block_refs.LN_OFFSET_MEASURED).  Measured on an MI355X: all three variants give the models' shares to every digit
    (0.99864 at H = 3072, r = 100; worst err / tol 0.74)."""
    B, L, split = br.LN_OFFSET_SHAPE
    data = br.ln_case_data(H, B, L, split, 0, kind, value)
    ref, mag = data[5], data[6]
    need = br.ln_offset_min_exact(H, kind, value)
    got = run_ln(ops, dev, data, split, variant, None)
    got8 = run_ln(ops, dev, data, split, variant, E5M2)
    print(f"ln_modulate H={H} {kind}={value} ln_variant={variant}: worst err/tol {worst_ratio(got, ref, mag, 2):.3f} (<= 1), "
          f"bit-exact {(got == ref).double().mean().item():.5f} (>= {need:.5f})")
    br.gate_ln_bf16(got, ref, mag, f"ln_modulate H={H} {kind}={value}", min_exact=need)
    q0, q1 = br.LN_QSCALES[E5M2]
    assert torch.equal(u8(got8), u8(br.ln_quant_ref(got, split, q0, q1, E5M2))), "the fp8 output is not quantise(own bf16 output)"
    br.gate_ln_f8(got8, br.ln_quant_ref(ref, split, q0, q1, E5M2), f"ln_modulate e5m2 H={H} {kind}={value}", y=ref, mag=mag)


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("H", [64, 520, 3072])
def test_ln_modulate_nan_stays_in_its_row(ops, dev, H, variant):
    B, L, split = 3, 9, 4
    data = br.ln_case_data(H, B, L, split)
    x = data[0].clone()
    x[1, 4, 5] = float("nan")
    for fmt in (None, E5M2):
        clean = run_ln(ops, dev, data, split, variant, fmt)
        got = run_ln(ops, dev, data, split, variant, fmt, x=x)
        assert bool(torch.isnan(got[1, 4].float()).all()), "the row that holds a NaN is not NaN throughout"
        keep = torch.ones(B, L, dtype=torch.bool)
        keep[1, 4] = False
        assert torch.equal(u8(got[keep]), u8(clean[keep])), "a NaN in one row changed another row"


PAIR_CASES = [(H, shape, v, f) for H in (64, 512, 3072) for shape in ((2, 42, 13), (2, 5, 2), (64, 42, 13)) for v, f in ((2, E5M2), (3, E5M2), (2, E4M3))]


@pytest.mark.parametrize("H,shape,variant,fmt", PAIR_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_ln_modulate_row_pair_layout(ops, dev, H, shape, variant, fmt):
    """out_pairs: the fp8 rows 2r, 2r + 1 of the B * L rows interleaved in 64-byte chunks.  unpair_rows of it must be the plain fp8 output,
    byte for byte; (2, 5, 2) has odd L, so a pair holds the last row of batch 0 and the first of batch 1.  The buffer ends in sentinel rows."""
    from fluxmi import _lib

    B, L, split = shape
    data = br.ln_case_data(H, B, L, split)
    plain = run_ln(ops, dev, data, split, variant, fmt)
    x, sh0, sc0, sh1, sc1 = (t.to(dev) for t in data[:5])
    obuf = sentinel_bytes(B * L + 2, H, dev)
    out = obuf.view(br.F8T[fmt])[:B * L].view(B, L, H)
    q = [torch.tensor(s, device=dev) for s in br.LN_QSCALES[fmt]]
    with _lib.tuning(ln_variant=variant):
        ops.ln_modulate(x, sh0, sc0, sh1, sc1, split=split, q_scale0=q[0], q_scale1=q[1], fmt=fmt, out=out, out_pairs=True)
    un = ops.unpair_rows(obuf[:B * L])
    torch.cuda.synchronize()
    assert torch.equal(un.cpu(), u8(plain).view(B * L, H)), "unpair_rows(out_pairs output) differs from the plain fp8 output"
    assert torch.equal(obuf[:B * L].cpu(), br.pair_rows_ref(u8(plain).view(B * L, H))), "the paired output is not pair_rows of the plain one"
    assert_sentinel(obuf[B * L:].view(torch.bfloat16), "ln_modulate out_pairs, rows past B * L")


@pytest.mark.parametrize("why", ["bf16_output", "odd_rows", "H_not_64", "ln_variant_1", "ldo_not_H"])
def test_ln_modulate_row_pair_refusals(ops, dev, why):
    from fluxmi import _lib

    H, (B, L, split) = (520 if why == "H_not_64" else 64), ((1, 7, 3) if why == "odd_rows" else (2, 5, 2))
    x, sh0, sc0, sh1, sc1 = (t.to(dev) for t in br.ln_inputs(B, L, H, 1))
    fp8 = why != "bf16_output"
    ow = H + 64 if why == "ldo_not_H" else H
    obuf = sentinel_bytes(B * L, ow * (1 if fp8 else 2), dev)
    out = obuf.view(torch.float8_e5m2 if fp8 else torch.bfloat16).view(B, L, ow)[:, :, :H]
    q = torch.tensor(900.0, device=dev) if fp8 else None
    with _lib.tuning(ln_variant=1 if why == "ln_variant_1" else 2):
        with pytest.raises(RuntimeError, match="row-pair output layout"):
            ops.ln_modulate(x, sh0, sc0, sh1, sc1, split=split, q_scale0=q, out=out, out_pairs=True)
    torch.cuda.synchronize()
    assert_sentinel(obuf.view(torch.bfloat16), f"ln_modulate out after the refusal ({why})")


# ---- qkv_rope ------------------------------------------------------------------------------------------------------------------
def run_qkv(ops, dev, data, H, split, skip_q, k_f16, ld_extra):
    """one launch into guarded Q / K / V^T -> (Q or None, K, VT) on the host"""
    qkv, pe, s = data[:3]
    B, L, _ = qkv.shape
    Lp = (L + 63) // 64 * 64
    full = sentinel_like((B, L, 3 * H * 128 + ld_extra), dev)
    full[..., :3 * H * 128] = qkv.to(dev)
    Q, fq = guarded((B, H, L, 128), torch.bfloat16, dev)
    K, fk = guarded((B, H, L, 128), torch.float16 if k_f16 else torch.bfloat16, dev)
    VT, fv = guarded((B, H, 128, Lp), torch.bfloat16, dev)
    sd = [t.to(dev) for t in s]
    r = ops.qkv_rope(full[..., :3 * H * 128], pe.to(dev), sd[0], sd[1], sd[2], sd[3], split=split, heads=H, skip_q=skip_q, k_f16=k_f16,
                     out=(Q, K, VT))
    torch.cuda.synchronize()
    assert r[0] is None if skip_q else r[0] is Q
    n = B * H * L * 128
    assert_guards(fq, n, "Q"), assert_guards(fk, n, "K"), assert_guards(fv, B * H * 128 * Lp, "V^T")
    if skip_q:
        assert_sentinel(Q, "Q under skip_q")
    return (None if skip_q else Q.cpu()), K.cpu(), VT.cpu()


@pytest.mark.parametrize("mode", list(br.QKV_MODES))
@pytest.mark.parametrize("case", br.QKV_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_qkv_rope(ops, dev, case, mode):
    """Every mode of fluxmi_k_qkv_rope at both row strides.  Q / K against the fp64 reference, V^T bit for bit (padding keys zero); K and V^T
    of a run without Q are the default run's bits; fp16 K is the fp16 of the default run's bf16 K, exactly.
    Measured on an MI355X: bit-exact share >= 0.99997 everywhere; the largest distance in plain ulps is 8 (K at (1, 24, 97, 64)), 4 at
    (2, 3, 200, 72) and 2 at (3, 2, 130, 129), each where the rotation cancels and inside one ulp at its magnitude (block_refs.gate_qk)."""
    B, H, L, split = case
    skip_q, k_f16 = br.QKV_MODES[mode]
    for ld_extra in br.QKV_LD_EXTRA:
        Qs, Ks, Qr, Kr, mq, mk = [], [], [], [], [], []
        for rep in range(br.reps_for(B * H * L * 128)):
            data = br.qkv_case_data(B, H, L, split, ld_extra, rep)
            Q, K, VT = run_qkv(ops, dev, data, H, split, skip_q, k_f16, ld_extra)
            br.gate_vt(VT, data[5], f"qkv_rope {case} {mode}")
            pad = br.vt_key_order(VT.shape[-1]) >= L
            assert not bool(VT[..., pad].any()), "V^T: a padding key is not zero"
            if mode != "default" and rep == 0:
                Qd, Kd, VTd = run_qkv(ops, dev, data, H, split, False, False, ld_extra)
                assert torch.equal(bits(VT), bits(VTd)), f"qkv_rope {mode}: V^T differs from the default run's"
                assert torch.equal(bits(K), bits(Kd.float().half() if k_f16 else Kd)), f"qkv_rope {mode}: K is not the default run's" + (" as fp16" if k_f16 else "")
                if Q is not None:
                    assert torch.equal(bits(Q), bits(Qd)), f"qkv_rope {mode}: Q differs from the default run's"
            if Q is not None:
                Qs.append(Q.reshape(-1)), Qr.append(data[3].reshape(-1)), mq.append(data[6].reshape(-1))
            Ks.append(K.reshape(-1)), Kr.append(data[4].reshape(-1)), mk.append(data[7].reshape(-1))
        K, Kref, mkk = torch.cat(Ks), torch.cat(Kr), torch.cat(mk)
        what = f"qkv_rope {case} {mode} ld=3*H*128+{ld_extra}"
        line = what + ":"
        if Qs:
            Q, Qref, mqq = torch.cat(Qs), torch.cat(Qr), torch.cat(mq)
            line += f" Q max ulp {br.max_ulp(Q, Qref)}, exact {(Q == Qref).double().mean().item():.5f};"
        Kb = K.float().bfloat16() if k_f16 else K
        print(line + f" K max ulp {br.max_ulp(Kb, Kref)}, exact {(Kb == Kref).double().mean().item():.5f} (>= 0.999) over {K.numel()} values; V^T bit-exact")
        if Qs:
            br.gate_qk(Q, Qref, mqq, what + " Q")
        if k_f16:
            br.gate_k_f16(K, Kref, mkk, what + " K fp16")
        else:
            br.gate_qk(K, Kref, mkk, what + " K")


@pytest.mark.parametrize("why", ["Lp_not_64", "ld_not_8"])
def test_qkv_rope_refusals(ops, dev, why):
    B, H, L, split = 1, 2, 33, 8
    qkv, pe, s = br.qkv_inputs(B, H, L, 3)
    ld = 3 * H * 128 + (4 if why == "ld_not_8" else 0)
    full = sentinel_like((B, L, ld), dev)
    full[..., :3 * H * 128] = qkv.to(dev)
    Lp = 33 if why == "Lp_not_64" else 64
    Q, fq = guarded((B, H, L, 128), torch.bfloat16, dev)
    K, fk = guarded((B, H, L, 128), torch.bfloat16, dev)
    VT, fv = guarded((B, H, 128, Lp), torch.bfloat16, dev)
    sd = [t.to(dev) for t in s]
    with pytest.raises(RuntimeError, match="multiple of 64" if why == "Lp_not_64" else "multiple of 8"):
        ops.qkv_rope(full[..., :3 * H * 128], pe.to(dev), sd[0], sd[1], sd[2], sd[3], split=split, heads=H, out=(Q, K, VT))
    torch.cuda.synchronize()
    for t, name in ((fq, "Q"), (fk, "K"), (fv, "V^T")):
        assert_sentinel(t.view(torch.bfloat16), f"{name} after the refusal ({why})")


# ---- the exact chains ----------------------------------------------------------------------------------------------------------
def col_slice(t, extra, off, dev, rows_extra=2):
    """t [B, L, H] (or [R, H]) on the host -> the same values as a column slice [.., off:off + H] of a sentinel buffer H + extra wide with
    spare rows; returns (view, buffer)"""
    t3 = t if t.dim() == 3 else t[None]
    B, L, H = t3.shape
    buf = sentinel_like((B * L + rows_extra, H + extra), dev)
    v = buf[:B * L].view(B, L, H + extra)[:, :, off:off + H]
    v.copy_(t3.to(dev))
    return (v if t.dim() == 3 else v[0]), buf


def check_slice_untouched(buf, before, B, L, H, extra, off, what):
    assert_only_written(buf.view(torch.uint8), before.view(torch.uint8),
                        lambda t: t[:B * L].view(B, L, (H + extra) * 2)[:, :, off * 2:(off + H) * 2], what)


@pytest.mark.parametrize("B,L,H", [(3, 7, 264), (2, 24, 256), (2, 300, 3072)])
def test_gate_residual_strided(ops, dev, B, L, H):
    """x, y and out are slices of three buffers of three widths (the engine calls the kernel that way); gate is a slice of a [B, 3H] table"""
    g = torch.Generator().manual_seed(br.seed_of("gate", B, L, H))
    x, y = torch.randn(B, L, H, generator=g).bfloat16(), (torch.randn(B, L, H, generator=g) * 3).bfloat16()
    table = torch.randn(B, 3 * H, generator=g).bfloat16()
    gate = table[:, H:2 * H]
    ref = br.gate_residual_ref(x, y, gate)
    xv, _ = col_slice(x, 8, 0, dev)
    yv, _ = col_slice(y, 16, 8, dev)
    ov, obuf = col_slice(torch.zeros(B, L, H).bfloat16(), 24, 16, dev)
    obuf.view(torch.int16).fill_(br.SENTINEL)
    before = obuf.clone()
    r = ops.gate_residual(xv, yv, table.to(dev)[:, H:2 * H], out=ov)
    torch.cuda.synchronize()
    assert r is ov and torch.equal(bits(ov.cpu()), bits(ref)), "gate_residual (strided) differs from bf16(x + bf16(gate * y))"
    check_slice_untouched(obuf, before, B, L, H, 24, 16, "gate_residual out")
    dense = ops.gate_residual(x.to(dev), y.to(dev), gate.contiguous().to(dev))
    assert torch.equal(bits(dense.cpu()), bits(ref))
    print(f"gate_residual B={B} L={L} H={H}: bit-exact, dense and strided")


@pytest.mark.parametrize("n", [8, 2040, 2048 * 256 + 8])
def test_add_and_euler(ops, dev, n):
    g = torch.Generator().manual_seed(br.seed_of("add", n))
    a, b = torch.randn(n, generator=g).bfloat16(), (torch.randn(n, generator=g) * 2).bfloat16()
    z, fz = guarded((n,), torch.bfloat16, dev)
    assert ops.add(a.to(dev), b.to(dev), out=z) is z
    torch.cuda.synchronize()
    assert torch.equal(bits(z.cpu()), bits(br.add_ref(a, b))), f"add n={n}"
    assert_guards(fz, n, "add")
    for dt in (0.9762182831764221 - 0.9884144067764282, -1.0 / 3.0):
        img, fi = guarded((n,), torch.bfloat16, dev)
        img.copy_(a.to(dev))
        ops.euler_(img, b.to(dev), dt)
        torch.cuda.synchronize()
        assert torch.equal(bits(img.cpu()), bits(br.euler_ref(a, b, dt))), f"euler_ n={n} dt={dt}"
        assert_guards(fi, n, "euler_")
    print(f"add / euler_ n={n}: bit-exact")


@pytest.mark.parametrize("rows,nb,cols", [(7, 3, 264), (1, 1, 8), (513, 4, 3072), (5, 8, 64)])
def test_add_bcast(ops, dev, rows, nb, cols):
    g = torch.Generator().manual_seed(br.seed_of("bcast", rows, nb, cols))
    a, b = torch.randn(rows, cols, generator=g).bfloat16(), torch.randn(nb, cols, generator=g).bfloat16()
    z, fz = guarded((rows, cols), torch.bfloat16, dev)
    ops.add_bcast(a.to(dev), b.to(dev), out=z)
    torch.cuda.synchronize()
    assert torch.equal(bits(z.cpu()), bits(br.add_bcast_ref(a, b))), f"add_bcast rows={rows} nb={nb}"
    assert_guards(fz, rows * cols, "add_bcast")
    print(f"add_bcast rows={rows} nb={nb} cols={cols}: bit-exact")


@pytest.mark.parametrize("mode", [0, 1])
def test_act_strided(ops, dev, mode):
    """a strided launch gives the dense launch's bits (test_act_tables gates those over every bf16 value) and writes nothing else"""
    R, C = 37, 264
    x = (torch.randn(R, C, generator=torch.Generator().manual_seed(11)) * 3).bfloat16()
    dense = ops.act(x.to(dev), mode).cpu()
    xv, _ = col_slice(x, 8, 8, dev)
    ov, obuf = col_slice(torch.zeros(R, C).bfloat16(), 40, 24, dev)
    obuf.view(torch.int16).fill_(br.SENTINEL)
    before = obuf.clone()
    assert ops.act(xv, mode, out=ov) is ov
    torch.cuda.synchronize()
    assert torch.equal(bits(ov.cpu()), bits(dense)), "act: strided and dense launches differ"
    check_slice_untouched(obuf, before, 1, R, C, 40, 24, "act out")
    want = torch.nn.functional.gelu(x.float(), approximate="tanh") if mode == 0 else torch.nn.functional.silu(x.float())
    assert float((dense.float() - want).abs().max()) <= 2.0 ** -7 * float(want.abs().max())


@pytest.mark.parametrize("rows,row_bytes", [(2, 64), (6, 64), (2, 192), (6, 192), (84, 3072)])
def test_pair_rows_and_back(ops, dev, rows, row_bytes):
    w = torch.randint(0, 256, (rows, row_bytes), generator=torch.Generator().manual_seed(rows * row_bytes), dtype=torch.uint8)
    p = ops.pair_rows(w.to(dev))
    assert torch.equal(p.cpu(), br.pair_rows_ref(w)), "pair_rows differs from [R/2][row_bytes/64][2][64]"
    assert torch.equal(ops.unpair_rows(p).cpu(), w), "unpair_rows(pair_rows(w)) is not w"
    w16 = w.view(torch.bfloat16)  # 2-byte elements: the same bytes
    assert torch.equal(u8(ops.pair_rows(w16.to(dev)).cpu()), br.pair_rows_ref(w))


# ---- tables --------------------------------------------------------------------------------------------------------------------
def test_rope_table_positions(ops, dev):
    """positions up to 1024 on each axis alone and on all three: cosf / sinf reduce arguments up to 1024 rad there"""
    ids = br.rope_ids()
    ref = br.rope_table_ref(ids)
    pe = ops.rope_table(ids.to(dev), br.AXES_DIM, br.THETA).cpu()
    print(f"rope_table {ids.shape[1]} rows, positions <= {int(ids.max())}: max ulp {br.max_ulp(pe, ref)} (<= 1), "
          f"bit-exact {(pe == ref).double().mean().item():.5f} (>= 0.999) over {pe.numel()} values")
    br.gate_rope(pe, ref, "rope_table")
    ids2 = torch.cat((ids, ids.flip(1)), 0)  # two batch elements, other rows in each
    pe2 = ops.rope_table(ids2.to(dev), br.AXES_DIM, br.THETA).cpu()
    assert torch.equal(bits(pe2[0]), bits(pe[0])) and torch.equal(bits(pe2[1]), bits(pe[0].flip(0)))


def test_timestep_embedding_every_bf16_t(ops, dev):
    t = br.timestep_values()
    ref = br.timestep_embedding_ref(t)
    got = ops.timestep_embedding(t.to(dev), br.timestep_freqs().to(dev)).cpu()
    print(f"timestep_embedding {t.numel()} values of t: max ulp {br.max_ulp(got, ref)} (<= 1), "
          f"bit-exact {(got == ref).double().mean().item():.5f} (>= 0.995) over {got.numel()} values")
    br.gate_timestep(got, ref, "timestep_embedding")
    assert torch.equal(br.timestep_freqs(), ops.timestep_freqs_host())
