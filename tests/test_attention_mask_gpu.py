"""Token-group masks of the flow attention (fluxmi_attention_grouped / _rawq_grouped; csrc/attention2.hip MASKED) on the GPU, against the
per-element gate of tests/attention_mask_ref.py: F.scaled_dot_product_attention(q, k, v, attn_mask=allowed) in fp64 and the working-
precision model, nothing measured on the kernel.  B <= 2, H = 2; folded (fp16 K) and bf16-K builds; bf16 and fp8 outputs (the latter also
in the row-pair layout); the Q and the raw-Q entries."""
import pytest
import torch

import attention_mask_ref as mr
import attention_ref as ar
import flux_oracle as fo

pytestmark = pytest.mark.gpu

E4M3, E5M2 = 0, 1
F8T = {E4M3: torch.float8_e4m3fn, E5M2: torch.float8_e5m2}
F8MAX = {E4M3: 448.0, E5M2: 57344.0}
F8_SCALES = {E5M2: (3000.0, 40000.0), E4M3: (200.0, 900.0)}
H = 2


@pytest.fixture(scope="module")
def ops(dev):
    from fluxmi import ops as _ops

    return _ops


def vt_layout(v, L):
    """V^T in the kernel's layout (transposed, bit 2 <-> bit 3 of the key index inside every 16-key group exchanged, zero padded to 64)"""
    B, Hh = v.shape[:2]
    Lp = (L + 63) // 64 * 64
    pos = torch.arange(Lp)
    j = pos % 16
    key = (pos // 16) * 16 + ((j & 3) | (((j >> 2) & 1) << 3) | (((j >> 3) & 1) << 2))
    vpad = torch.zeros(B, Hh, Lp, 128, dtype=torch.bfloat16)
    vpad[:, :, :L] = v
    return vpad[:, :, key].transpose(-1, -2).contiguous()


def region_table(L):
    """(a): a text / region layout from flux_pipeline.build_region_groups whose segment edges lie off the 32- and 64-key boundaries"""
    from flux_pipeline import build_region_groups

    h, w, nb = {64: (5, 5, 7), 100: (6, 8, 20), 333: (15, 17, 46), 448: (20, 19, 36), 640: (24, 24, 32), 3264: (56, 57, 40)}[L]
    ys, xs = torch.arange(h)[:, None], torch.arange(w)[None, :]
    r1 = (xs < (2 * w) // 3) & (ys < (3 * h) // 4)  # two overlapping boxes that leave a margin uncovered
    r2 = (xs >= w // 3) & (ys >= h // 4)
    t = build_region_groups(nb, 16, torch.stack((r1, r2)))
    assert t.numel() == L
    return t.to(torch.int64)


def tables_for(L, which):
    fn = dict(a=region_table, b=mr.table_first_tiles_masked, c=mr.table_last_tiles_masked, d=mr.table_stripes)
    if which == "e":  # different tables for the two samples of a batch
        return torch.stack((region_table(L), mr.table_stripes(L)))
    return fn[which](L)[None]


def f8_quantised(out, split, fmt):
    s0, s1 = (torch.tensor(s) for s in F8_SCALES[fmt])
    return torch.cat((fo.to_fp8_saturated(out[:, :split], s0, F8MAX[fmt]).to(F8T[fmt]), fo.to_fp8_saturated(out[:, split:], s1, F8MAX[fmt]).to(F8T[fmt])), 1)


@pytest.mark.parametrize("L", [64, 333, 640])
def test_all_allowed_table_is_the_dense_launch(ops, dev, L):
    """a table that admits everything (keys spread over all 16 groups) == the dense launch, bit for bit: bf16 and fp8 outputs, both K formats"""
    B = 2
    q, k, v = ar.attention_inputs("randn", B, H, L, seed=31)
    d = lambda t: t.to(dev)
    tab = d(mr.to_i32(mr.table_all(L)[None].expand(B, L).contiguous()))
    s0, s1 = (d(torch.tensor(s)) for s in F8_SCALES[E5M2])
    for fold in (False, True):
        qd, kd, vd = d(q), d(k.half() if fold else k), d(vt_layout(v, L))
        dense, masked = ops.attention(qd, kd, vd), ops.attention(qd, kd, vd, groups=tab)
        assert torch.equal(dense.view(torch.int16), masked.view(torch.int16)), f"L={L} fold={fold}: all-allowed table differs from dense"
        dense8 = ops.attention(qd, kd, vd, q_scale0=s0, q_scale1=s1, split=L // 3)
        masked8 = ops.attention(qd, kd, vd, q_scale0=s0, q_scale1=s1, split=L // 3, groups=tab)
        assert torch.equal(dense8.view(torch.uint8), masked8.view(torch.uint8)), f"L={L} fold={fold}: fp8 all-allowed table differs from dense"


def _gate_case(ops, dev, L, family, which, B):
    q, k, v = ar.attention_inputs(family, B, H, L, seed=33)
    tab = tables_for(L, which)
    if tab.shape[0] != B:
        tab = tab.expand(B, L).contiguous()
    assert mr.self_admitting(tab)
    allowed = mr.allowed_of(tab)
    ref_A = mr.attention_ref64_masked(q, k, v, allowed)
    d = lambda t: t.to(dev)
    tabd = d(mr.to_i32(tab))
    stats = {}
    for fold in (False, True):
        gate = mr.masked_gate(q, k, v, allowed, fold, ref_A=ref_A)
        what = f"masked L={L} {family} table ({which}) {'fp16' if fold else 'bf16'} K"
        qd, kd, vd = d(q), d(k.half() if fold else k), d(vt_layout(v, L))
        out = ops.attention(qd, kd, vd, groups=tabd).cpu()
        stats[fold] = ar.assert_attention_close(out, q, k, v, fold, what, gate=gate)
        zero_bound = gate["bound"] == 0  # columns with no visible V: exactly 0 (assert_attention_close demands it; said again in words)
        assert (out[zero_bound].float() == 0).all(), f"{what}: a column whose admitted keys carry no V is not exactly 0"
        # fp8 output == quantise(own bf16 output), plain rows and the row-pair layout
        for fmt in (E5M2, E4M3):
            s0, s1 = (d(torch.tensor(s)) for s in F8_SCALES[fmt])
            want = f8_quantised(out, L // 3, fmt)
            got8 = ops.attention(qd, kd, vd, q_scale0=s0, q_scale1=s1, split=L // 3, fmt=fmt, groups=tabd)
            assert not (got8.cpu().float() != want.float()).any(), f"{what} fmt={fmt}: fp8 output != quantise(bf16 output)"
            if (B * L) % 2 == 0 and L % 2 == 0:
                pairs = ops.attention(qd, kd, vd, q_scale0=s0, q_scale1=s1, split=L // 3, fmt=fmt, groups=tabd, out_pairs=True)
                rows = ops.unpair_rows(pairs.view(torch.uint8).reshape(B * L, H * 128)).view(B, L, H * 128)
                assert torch.equal(rows, got8.view(torch.uint8)), f"{what} fmt={fmt}: the row-pair layout holds other bytes"
    return stats


LS, FAMILIES = (64, 100, 333, 448, 3264), ("randn", "pos", "probe_last")
# every table at every L over every family; (b) is the one the issue states with `pos` inputs only
CASES = [(L, fam, which) for which in "abcde" for L in LS for fam in (("pos",) if which == "b" else FAMILIES)]


@pytest.mark.parametrize("L,family,which", CASES)
def test_masked_attention_gate(ops, dev, L, family, which):
    """(a) region layout, (b) first two key tiles entirely masked for half the rows with `pos` inputs (the rows start from an empty softmax
    state and meet their first admitted score in a later tile: the rescale-to-zero path), (c) last tiles entirely masked, (d) sixteen
    one-key-in-sixteen stripes, (e) another table per sample"""
    _gate_case(ops, dev, L, family, which, B=2 if which == "e" else 1)


@pytest.mark.parametrize("L,Lt", [(100, 36), (333, 78)])
def test_masked_rawq_entry(ops, dev, L, Lt):
    """the raw-Q entry (QKNorm + RoPE on load) under a region table: through the gate on the oracle's normalised + rotated q, k, and the
    all-allowed table == the dense raw-Q launch bit for bit"""
    torch.manual_seed(92)
    B = 2
    qkv = torch.randn(B, L, 3 * H * 128 + 64).bfloat16()
    s = [(1 + 0.1 * torch.randn(128)).bfloat16() for _ in range(4)]
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
    q_ref, k_ref = q_ref.bfloat16(), ar.flush_k(k_ref.bfloat16())
    tab = torch.stack((region_table(L), mr.table_two_regions(L)))
    allowed = mr.allowed_of(tab)
    ref_A = mr.attention_ref64_masked(q_ref, k_ref, v, allowed)
    d = lambda t: t.to(dev)
    qkv_d = d(qkv)[..., : 3 * H * 128]
    tabd, alld = d(mr.to_i32(tab)), d(mr.to_i32(mr.table_all(L)[None].expand(B, L).contiguous()))
    for f16 in (False, True):
        _, K, VT = ops.qkv_rope(qkv_d, d(pe), d(s[0]), d(s[1]), d(s[2]), d(s[3]), split=Lt, heads=H, k_f16=f16, skip_q=True)
        run = lambda g: ops.attention_rawq(qkv_d, d(pe), d(s[0]), K, VT, qn_scale1=d(s[2]), split=Lt, groups=g)
        assert torch.equal(run(None).view(torch.int16), run(alld).view(torch.int16)), f"raw-Q L={L} f16={f16}: all-allowed differs from dense"
        gate = mr.masked_gate(q_ref, k_ref, v, allowed, f16, ref_A=ref_A)
        # the raw-Q path normalises and rotates Q itself (a rare bf16 ulp against the oracle's q): the gate's own margin covers it
        ar.assert_attention_close(run(tabd).cpu(), q_ref, k_ref, v, f16, f"masked raw-Q L={L} f16={f16}", gate=gate)


def test_masked_launches_take_no_plan(ops, dev):
    """At a shape where ops.attention_plan returns a plan, a masked launch runs one workgroup per task under every attn_split: its bits do
    not depend on the knob (the dense launch's do: the balanced grid merges partial softmax states), and it passes the gate."""
    from fluxmi import _lib

    B, L, Hh = 1, 1100, 8  # a shape of test_attention_balanced_grid (tests/test_ops_gpu.py): a single partial round, which attn_split = 2 bins
    plan = ops.attention_plan(B, L, Hh)
    assert plan is not None, "the shape was chosen to have a balanced-grid plan"
    q, k, v = ar.attention_inputs("randn", B, Hh, L, seed=35)
    tab = mr.table_two_regions(L)[None]
    d = lambda t: t.to(dev)
    qd, kd, vd, tabd = d(q), d(k.half()), d(vt_layout(v, L)), d(mr.to_i32(tab))
    outs, dense = {}, {}
    for split in (0, 2):
        with _lib.tuning(attn_split=split):
            outs[split] = ops.attention(qd, kd, vd, groups=tabd).cpu()
            dense[split] = ops.attention(qd, kd, vd).cpu()
    assert torch.equal(outs[0].view(torch.int16), outs[2].view(torch.int16)), "a masked launch changed with attn_split: it took a plan"
    assert not torch.equal(dense[0].view(torch.int16), dense[2].view(torch.int16)), "the dense launch at this shape should take the plan (the control)"
    allowed = mr.allowed_of(tab)
    hs = [0, Hh - 1]  # the first head and the last one (a leftover task, cut into pieces in the dense launch)
    mr.assert_masked_close(outs[2].view(B, L, Hh, 128)[:, :, hs].reshape(B, L, 256), q[:, hs], k[:, hs], v[:, hs], allowed, True, "masked, attn_split=2")


def test_stale_tables(ops, dev):
    """two different tables alternate between launches on the same buffers (the table is device data read per launch; the staged copy in
    LDS is rebuilt by every workgroup): each launch equals the first launch with its table"""
    B, L = 2, 333
    q, k, v = ar.attention_inputs("randn", B, H, L, seed=36)
    d = lambda t: t.to(dev)
    qd, kd, vd = d(q), d(k.half()), d(vt_layout(v, L))
    t1 = mr.to_i32(torch.stack((region_table(L), mr.table_stripes(L))))
    t2 = mr.to_i32(torch.stack((mr.table_first_tiles_masked(L), mr.table_two_regions(L))))
    buf, out = d(t1.clone()), torch.empty(B, L, H * 128, dtype=torch.bfloat16, device=dev)
    first = {}
    for rnd in range(3):
        for name, t in (("t1", t1), ("t2", t2)):
            buf.copy_(d(t))
            got = ops.attention(qd, kd, vd, out=out, groups=buf).cpu().clone()
            if rnd == 0:
                first[name] = got
            assert torch.equal(got.view(torch.int16), first[name].view(torch.int16)), f"round {rnd} table {name}: a stale table was read"
    assert not torch.equal(first["t1"].view(torch.int16), first["t2"].view(torch.int16))
    mr.assert_masked_close(first["t2"], q, k, v, mr.allowed_of(t2), True, "stale tables: t2")


def test_self_admission_is_checked(ops, dev):
    B, L = 1, 64
    q, k, v = ar.attention_inputs("randn", B, H, L, seed=37)
    d = lambda t: t.to(dev)
    bad = mr.table_stripes(L)[None].clone()
    bad[0, 5] = mr.desc(torch.tensor(5), torch.tensor(1 << 6))  # admits group 6 only
    with pytest.raises(ValueError, match="own key group"):
        ops.attention(d(q), d(k), d(vt_layout(v, L)), groups=d(mr.to_i32(bad)))


def test_scores_at_the_documented_lower_end(ops, dev):
    """include/fluxmi.h: admitted scores must stay above the masked rows' starting maximum + 126 in the exp2 domain.  Every score of this
    case lies within a few units of that lower end (a common vector of opposite sign in q and k), half the rows start with two masked
    tiles; the output passes the gate like any other"""
    import math

    L, level = 200, ops.ATTN_MASK_FLOOR + 126
    g = torch.Generator().manual_seed(39)
    a = math.sqrt(-level / float(ar.SCALE_LOG2) / 128)
    q = (a + 0.1 * torch.randn(1, H, L, 128, generator=g)).bfloat16()
    k = ar.flush_k((-a + 0.1 * torch.randn(1, H, L, 128, generator=g)).bfloat16())
    v = torch.randn(1, H, L, 128, generator=g).bfloat16()
    s = (q.float() @ k.float().transpose(-1, -2)) * ar.SCALE_LOG2
    assert level - 26 < float(s.min()) and float(s.max()) < level + 26
    tab = mr.table_first_tiles_masked(L)[None]
    allowed = mr.allowed_of(tab)
    ref_A = mr.attention_ref64_masked(q, k, v, allowed)
    d = lambda t: t.to(dev)
    for fold in (False, True):
        out = ops.attention(d(q), d(k.half() if fold else k), d(vt_layout(v, L)), groups=d(mr.to_i32(tab))).cpu()
        ar.assert_attention_close(out, q, k, v, fold, f"scores near {level:.0f}, {'fp16' if fold else 'bf16'} K", gate=mr.masked_gate(q, k, v, allowed, fold, ref_A=ref_A))
