"""CPU companion of tests/test_block_kernels_gpu.py: proves the gates that module applies to the block glue kernels.

For every op the gate is fed (a) the fp64 reference itself, (b) a torch fp32 model written in the kernel's order of operations
(tests/block_refs.py: the one-wave and the pairwise summation of ln_modulate, the 16-lane butterfly of qkv_rope, torch's fp32 cos / sin
for the tables), which must pass: the gates are attainable in fp32, so a kernel that misses one is wrong and not merely single precision;
and (c) seeded WRONG variants of the reference (`mut=`), each of which must be rejected at the case named beside it.
"""
import pytest
import torch

import block_refs as br
from block_refs import E4M3, E5M2


def rejected(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


def pooled_ln(H, B, L, split, kind=None, value=None):
    """the launches of one case, as the GPU module pools them: lists of ln_case_data tuples"""
    return [br.ln_case_data(H, B, L, split, rep, kind, value) for rep in range(br.reps_for(B * L * H))]


def cat_ln(datas, fn):
    return torch.cat([fn(*d).reshape(-1) for d in datas])


LN_UNIQUE = sorted({c[:4] for c in br.LN_CASES})


# ---- the tables themselves -----------------------------------------------------------------------------------------------------
def test_case_tables_cover_every_arm_and_are_pooled():
    hs, shapes = {c[0] for c in br.LN_CASES}, {c[1:4] for c in br.LN_CASES}
    assert hs == set(br.LN_HS) and shapes == set(br.LN_SHAPES)
    for H in br.LN_HS:  # every (H, variant, format), hence every instantiation of the launcher: 2 kernels x NCH x format x FULL / guarded
        assert {(c[4], c[5]) for c in br.LN_CASES if c[0] == H} == {(v, f) for v in br.LN_VARIANTS for f in br.FMTS}
        assert {c[6] for c in br.LN_CASES if c[0] == H} == {True, False}, "dense and strided at every H"
    arms = {(br.ln_arm(c[0], c[4]), c[5]) for c in br.LN_CASES}
    want = {f"onewave-nch{n}" for n in (1, 2, 4, 6, 8)} | {f"stream-nch{n}-{g}" for n in (1, 2, 4, 6) for g in ("full", "guarded")}
    assert {a for a, _ in arms} == want and all((a, f) in arms for a in want for f in br.FMTS)
    for H in (64, 520, 3072):
        for shape in br.LN_SHAPES:
            assert {c[4] for c in br.LN_CASES if c[0] == H and c[1:4] == shape} & {1, 2}, (H, shape)
    for c in br.LN_CASES:  # the pooling rule
        assert br.reps_for(c[1] * c[2] * c[0]) * c[1] * c[2] * c[0] >= br.POOL
    for B, H, L, split in br.QKV_CASES:
        assert br.reps_for(B * H * L * 128) * B * H * L * 128 >= br.POOL
    launches = sum(br.reps_for(c[1] * c[2] * c[0]) * (1 if c[5] == "bf16" else 2) for c in br.LN_CASES)
    assert launches <= 500, f"{launches} ln_modulate launches (128 of them are the one-row shapes at H = 64)"
    assert br.rope_table_ref(br.rope_ids()).numel() >= br.POOL and br.timestep_values().numel() * 256 >= br.POOL


# ---- ln_modulate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,B,L,split", LN_UNIQUE, ids=lambda v: str(v))
def test_ln_gates_accept_the_reference_and_the_fp32_models(H, B, L, split):
    datas = pooled_ln(H, B, L, split)
    ref = cat_ln(datas, lambda *d: d[5])
    mag = cat_ln(datas, lambda *d: d[6])
    br.gate_ln_bf16(ref, ref, mag, "reference")
    for order in ("one_wave", "pairwise"):
        got = [br.ln_modulate_fp32(*d[:5], split, order) for d in datas]
        ex = br.gate_ln_bf16(torch.cat([g.reshape(-1) for g in got]), ref, mag, f"fp32 {order} H={H} {(B, L, split)}")
        assert ex >= 0.999
        for fmt in (E5M2, E4M3):
            q0, q1 = br.LN_QSCALES[fmt]
            gq = torch.cat([br.ln_quant_ref(g, split, q0, q1, fmt).reshape(-1) for g in got])
            rq = torch.cat([br.ln_quant_ref(d[5], split, q0, q1, fmt).reshape(-1) for d in datas])
            br.gate_ln_f8(gq, rq, f"fp32 {order} fp8 {fmt} H={H}", y=ref, mag=mag)


@pytest.mark.parametrize("H,kind,value", br.LN_OFFSETS)
def test_ln_offset_gate_is_the_fp32_models_minus_a_margin(H, kind, value):
    """min_exact of the DC-offset cases is derived from these very measurements (block_refs.LN_OFFSET_MEASURED); the 2-ulp bound is not moved"""
    B, L, split = br.LN_OFFSET_SHAPE
    x, sh0, sc0, sh1, sc1, ref, mag = br.ln_case_data(H, B, L, split, 0, kind, value)
    need = br.ln_offset_min_exact(H, kind, value)
    assert 0.99 <= need <= 0.999
    for i, order in enumerate(("one_wave", "pairwise")):
        got = br.ln_modulate_fp32(x, sh0, sc0, sh1, sc1, split, order)
        ex = br.gate_ln_bf16(got, ref, mag, f"fp32 {order} H={H} {kind}={value}", min_exact=need)
        print(f"ln_modulate fp32 {order} H={H} {kind}={value}: bit-exact {ex:.5f} (gate {need:.5f})")
        if (H, value) in br.LN_OFFSET_MEASURED and kind == "offset":
            assert abs(ex - br.LN_OFFSET_MEASURED[(H, value)][i]) <= 1e-3, "the recorded measurement is stale"
        q0, q1 = br.LN_QSCALES[E5M2]
        br.gate_ln_f8(br.ln_quant_ref(got, split, q0, q1, E5M2), br.ln_quant_ref(ref, split, q0, q1, E5M2), f"fp32 {order} e5m2 H={H} {kind}={value}",
                      y=ref, mag=mag)


LN_MUTANTS = [  # (mutant, H, (B, L, split), kind, value): the case at which the gate must reject it
    ("one_pass_var", 520, br.LN_OFFSET_SHAPE, "offset", 100), ("one_pass_var", 3072, br.LN_OFFSET_SHAPE, "offset", 100),
    ("scale_unrounded", 256, (3, 9, 4), None, None), ("scale_unrounded", 3072, (1, 7, 3), None, None),
    ("split_le", 520, (3, 9, 4), None, None), ("split_le", 64, (1, 1, 0), None, None), ("split_le", 3072, (2, 42, 13), None, None),
    ("batch_shift", 64, (2, 5, 2), None, None), ("batch_shift", 3072, (2, 42, 13), None, None),
    ("drop_last_8", 520, (2, 42, 13), None, None), ("drop_last_8", 3072, (2, 42, 13), None, None), ("drop_last_8", 64, (1, 7, 3), None, None),
]


@pytest.mark.parametrize("mut,H,shape,kind,value", LN_MUTANTS, ids=lambda v: str(v).replace(" ", ""))
def test_ln_gate_rejects_wrong_kernels(mut, H, shape, kind, value):
    B, L, split = shape
    datas = pooled_ln(H, B, L, split, kind, value)
    ref = cat_ln(datas, lambda *d: d[5])
    mag = cat_ln(datas, lambda *d: d[6])
    need = br.ln_offset_min_exact(H, kind, value) if kind else 0.999
    bad = torch.cat([br.ln_modulate_ref(*d[:5], split, mut=mut)[0].reshape(-1) for d in datas])
    rejected(br.gate_ln_bf16, bad, ref, mag, mut, min_exact=need)


@pytest.mark.parametrize("fmt", [E5M2, E4M3])
def test_ln_fp8_gate_rejects_the_other_streams_scale(fmt):
    B, L, split = 2, 42, 13
    ref = br.ln_case_data(520, B, L, split)[5]
    q0, q1 = br.LN_QSCALES[fmt]
    good = br.ln_quant_ref(ref, split, q0, q1, fmt)
    br.gate_ln_f8(good, good, "reference")
    rejected(br.gate_ln_f8, br.ln_quant_ref(ref, split, q0, q1, fmt, mut="wrong_q_stream"), good, "wrong_q_stream")
    sat = (good.float().abs() == br.F8MAX[fmt]).float().mean().item()
    assert sat > 0, "the scales are meant to reach the clamp"


# ---- qkv_rope ------------------------------------------------------------------------------------------------------------------
def pooled_qkv(B, H, L, split, ld_extra=0):
    return [br.qkv_case_data(B, H, L, split, ld_extra, rep) for rep in range(br.reps_for(B * H * L * 128))]


@pytest.mark.parametrize("B,H,L,split", br.QKV_CASES, ids=lambda v: str(v))
def test_qkv_gates_accept_the_reference_and_the_fp32_model(B, H, L, split):
    datas = pooled_qkv(B, H, L, split, 64)
    Qr = torch.cat([d[3].reshape(-1) for d in datas])
    Kr = torch.cat([d[4].reshape(-1) for d in datas])
    mq = torch.cat([d[6].reshape(-1) for d in datas])
    mk = torch.cat([d[7].reshape(-1) for d in datas])
    br.gate_qk(Qr, Qr, mq, "Q reference")
    got = [br.qkv_rope_fp32(d[0], d[1], d[2], H, split) for d in datas]
    br.gate_qk(torch.cat([g[0].reshape(-1) for g in got]), Qr, mq, f"fp32 Q {(B, H, L, split)}")
    br.gate_qk(torch.cat([g[1].reshape(-1) for g in got]), Kr, mk, f"fp32 K {(B, H, L, split)}")
    br.gate_k_f16(torch.cat([br.k_as_f16(g[1]).reshape(-1) for g in got]), Kr, mk, f"fp32 K as fp16 {(B, H, L, split)}")
    VT = datas[0][5]
    br.gate_vt(VT, VT, "V^T reference")
    Lp = VT.shape[-1]
    # the padding is zero.  With the key permutation that is "every storage column whose KEY is >= L", not "columns [L, Lp)": at L = 200
    # the columns 200..203 hold the keys 196..199 and the columns 196..199 are padding
    pad = br.vt_key_order(Lp) >= L
    assert Lp % 64 == 0 and Lp - L < 64 and int(pad.sum()) == Lp - L and not bool(VT[..., pad].any()) and bool(VT[..., ~pad].any())
    assert (L % 16 <= 4 or L % 16 >= 12) == bool((pad == (torch.arange(Lp) >= L)).all())
    # the sentinel columns of the wider row never reach the reference
    assert torch.isfinite(Qr.float()).all() and torch.isfinite(Kr.float()).all() and torch.isfinite(VT.float()).all()


QKV_MUTANTS = [  # (mutant, (B, H, L, split)): the case at which it must be rejected
    ("vt_unpermuted", (1, 2, 33, 8)), ("vt_unpermuted", (1, 1, 64, 64)), ("heads_swapped", (1, 2, 33, 8)), ("heads_swapped", (1, 24, 97, 64)),
    ("rotation_sign", (1, 1, 1, 0)), ("rotation_sign", (2, 3, 63, 0)), ("stream0_on_first_image_row", (1, 2, 65, 1)),
    ("stream0_on_first_image_row", (3, 2, 130, 129)), ("stream0_on_first_image_row", (1, 1, 1, 0)), ("pe_prev_token", (1, 2, 33, 8)),
    ("pe_prev_token", (2, 3, 200, 72)), ("f16_from_unrounded", (1, 2, 33, 8)), ("f16_from_unrounded", (1, 1, 1, 1)),
]


@pytest.mark.parametrize("mut,case", QKV_MUTANTS, ids=lambda v: str(v).replace(" ", ""))
def test_qkv_gate_rejects_wrong_kernels(mut, case):
    B, H, L, split = case
    datas = pooled_qkv(B, H, L, split)
    Qr = torch.cat([d[3].reshape(-1) for d in datas])
    Kr = torch.cat([d[4].reshape(-1) for d in datas])
    mq = torch.cat([d[6].reshape(-1) for d in datas])
    mk = torch.cat([d[7].reshape(-1) for d in datas])
    bad = [br.qkv_rope_ref(d[0], d[1], d[2], H, split, mut=None if mut == "f16_from_unrounded" else mut) for d in datas]
    if mut == "vt_unpermuted":
        rejected(br.gate_vt, bad[0][2], datas[0][5], mut)
    elif mut == "f16_from_unrounded":
        k16 = torch.cat([br.k_as_f16(b[1], b[3], mut=mut).reshape(-1) for b in bad])
        rejected(br.gate_k_f16, k16, Kr, mk, mut)
    else:
        rejected(br.gate_qk, torch.cat([b[0].reshape(-1) for b in bad]), Qr, mq, mut + " Q")
        rejected(br.gate_qk, torch.cat([b[1].reshape(-1) for b in bad]), Kr, mk, mut + " K")
        if mut == "heads_swapped":
            rejected(br.gate_vt, bad[0][2], datas[0][5], mut + " V^T")


# ---- the exact chains ----------------------------------------------------------------------------------------------------------
def test_exact_chain_references_are_torchs_bf16_expressions():
    g = torch.Generator().manual_seed(5)
    B, L, H = 3, 7, 264
    x, y = torch.randn(B, L, H, generator=g).bfloat16(), (torch.randn(B, L, H, generator=g) * 3).bfloat16()
    gate = torch.randn(B, H, generator=g).bfloat16()
    assert torch.equal(br.bits(br.gate_residual_ref(x, y, gate)), br.bits(x + gate[:, None] * y))
    assert torch.equal(br.bits(br.add_ref(x, y)), br.bits(x + y))
    a, b = x.reshape(B * L, H), y.reshape(B * L, H)[:4].contiguous()
    assert torch.equal(br.bits(br.add_bcast_ref(a, b)), br.bits(a + b.repeat(6, 1)[:B * L]))
    for dt in (0.9762182831764221 - 0.9884144067764282, -1.0 / 3.0, 0.0625):
        assert torch.equal(br.bits(br.euler_ref(x, y, dt)), br.bits(x + dt * y))
    # the product dt * pred rounds to fp32 BEFORE bf16: a reference that rounds the fp64 product once differs somewhere over all of bf16
    allv = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    allv = allv[torch.isfinite(allv)]
    dt = -1.0 / 3.0
    once = br.round_fp64_to_bf16(torch.zeros_like(allv).double() + br.rbf64(torch.tensor(dt, dtype=torch.float32).double() * allv.double()))
    assert torch.equal(br.bits(br.euler_ref(torch.zeros_like(allv), allv, dt)), br.bits(torch.zeros_like(allv) + dt * allv))
    print(f"euler_: single rounding of dt * pred differs from the fp32-then-bf16 chain at {(once != br.euler_ref(torch.zeros_like(allv), allv, dt)).sum().item()} of {allv.numel()} values")


@pytest.mark.parametrize("rows,row_bytes", [(2, 64), (6, 64), (2, 192), (6, 192)])
def test_pair_rows_reference_formula(rows, row_bytes):
    w = torch.arange(rows * row_bytes, dtype=torch.int32).remainder(251).to(torch.uint8).view(rows, row_bytes)
    p = br.pair_rows_ref(w).reshape(-1)
    for r in range(rows):
        for c in (0, 63, row_bytes - 64, row_bytes - 1):
            assert p[(r >> 1) * 2 * row_bytes + (r & 1) * 64 + (c >> 6) * 128 + (c & 63)] == w[r, c]  # common.h f8_act_off
    assert sorted(p.tolist()) == sorted(w.reshape(-1).tolist())


# ---- tables --------------------------------------------------------------------------------------------------------------------
def test_table_gates_accept_the_reference_and_torchs_fp32():
    ids = br.rope_ids()
    ref = br.rope_table_ref(ids)
    br.gate_rope(ref, ref, "rope reference")
    br.gate_rope(br.rope_table_ref(ids, fp32=True), ref, "rope fp32")
    assert float(ids.max()) == 1024.0 and ids.shape[1] == 4 * len(br.ROPE_POSITIONS)  # 511 and 1023 are 512 and 1024 in bf16
    # the positions matter: an angle formed in fp64 instead of the fp32 product is another function there
    om, ax = br.rope_omega()
    ang64 = ids.double()[..., ax] * om.double()
    wrong = br.round_fp64_to_bf16(torch.stack((torch.cos(ang64), torch.sin(ang64)), -1))
    big = ids[0, :, 0] >= 63
    br.gate_rope(wrong[:, ~big], ref[:, ~big], "fp64 angles at small positions")
    t = br.timestep_values()
    assert t.numel() == 0x3F81 + 4 and float(t[0x3F80]) == 1.0
    tref = br.timestep_embedding_ref(t)
    br.gate_timestep(tref, tref, "timestep reference")
    br.gate_timestep(br.timestep_embedding_ref(t, fp32=True), tref, "timestep fp32")
    # without the bf16 rounding of 1000 t the embedding is another function
    arg = (1000.0 * t.float())[:, None] * br.timestep_freqs()[None]
    rejected(br.gate_timestep, br.round_fp64_to_bf16(torch.cat((torch.cos(arg.double()), torch.sin(arg.double())), -1)), tref, "t unrounded")
