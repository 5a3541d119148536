"""CPU (no GPU): the GEMM placement tests test something.

tests/test_gemm_frames_gpu.py holds the HIP kernels to an fp64 reference on strided views inside sentinel frames (tests/gemm_refs.py).
Here, without a GPU: (1) a kernel written in torch that accumulates in fp32 and rounds once -- what a correct kernel does -- passes every
gate on every case, sentinels included, so the gates and the pooling of small cases are conditions a correct kernel meets; (2) the same
kernel made wrong in one named way (an ignored stride, a row stored at M, another group's weight, a dropped K-step, ...) is rejected, and
the test names the case that rejects it; (3) the launch planner keeps groups with different lda off the persistent kernel and plans the
other groups of a launch the same with or without an empty group; (4) fluxmi_gemm_grouped refuses strides and pointers the kernels'
vector accesses cannot take, by field name, before it launches anything (the refusal is host code: it runs here)."""

import pytest

import gemm_refs as gr


@pytest.mark.parametrize("case", gr.CASES, ids=gr.CASE_IDS)
def test_fp32_emulation_passes_every_gate(case):
    """torch's fp32 matmul on the identical operands, one rounding, stores through the frames' own strides: within the gate of the fp64
    reference (pooled to >= POOL outputs), every sentinel intact"""
    assert gr.pool_reps(case) * gr.outputs_of(case) >= gr.POOL
    gr.run_case(case, lambda c, prob, frames, rep: gr.emulate(c, prob, frames))


def test_every_launcher_and_family_is_in_the_list():
    names = {c.id.split("-")[0] for c in gr.CASES}
    assert names >= {"cfg2", "cfg15", "cfg13", "cfg16", "cfg17", "cfg18", "cfg20", "cfg21", "generic", "splitk2", "splitk3", "auto"}
    for cfg in gr.LAUNCHERS:
        mine = [c for c in gr.CASES if c.cfg == cfg]
        bm = gr.TILES[cfg]["bm"]
        assert {c.Ms for c in mine if len(c.Ms) == 1} >= {(1,), (bm - 1,), (bm,), (bm + 1,)}
        assert any(0 == c.Ms[0] for c in mine) and any(len(c.Ms) == 3 and c.Ms[1] == 0 for c in mine) and any(c.Ms[-1] == 0 for c in mine)
        assert any(c.bias[:2] == (True, False) for c in mine)
        assert cfg == 18 or any(len(set(c.lda_extra)) == 3 for c in mine)
        assert all(set(c.lda_extra) == {0} for c in mine if cfg == 18)
    # strides, offsets: multiples of 64 bytes
    for c in gr.CASES:
        eb = 1 if c.op == "f8" else 2
        assert all((c.K + 128 + e) * eb % 64 == 0 for e in c.lda_extra) and (c.N + 128) * 2 % 64 == 0 and (c.N + 64) * 2 % 64 == 0, c.id


@pytest.mark.parametrize("mutant", gr.MUTANTS)
def test_every_mutant_is_rejected(mutant):
    """one wrong kernel each; at least one case must fail it (gate or sentinels), and that case is named"""
    wants = {"ldr_is_ldc": lambda c: c.resid == "sep", "splitk_late": lambda c: c.cfg > gr.SPLITK0, "ignore_c2_col0": lambda c: c.epi == "split",
             "full_n_tile": lambda c: c.N < 256, "group0_w": lambda c: len(c.Ms) > 1, "group0_bias": lambda c: len(c.Ms) > 1,
             "group0_scale": lambda c: len(c.Ms) > 1 and c.op == "f8"}.get(mutant, lambda c: True)
    killers = []
    for case in [c for c in gr.CASES if wants(c)][:40]:
        try:
            gr.run_case(case, lambda c, prob, frames, rep: gr.emulate(c, prob, frames, mutant))
        except AssertionError as e:
            killers.append((case.id, str(e)[:160]))
            if len(killers) == 3:
                break
    assert killers, f"mutant {mutant} passes every case"
    print(f"mutant {mutant} rejected by: " + "; ".join(f"{k} [{why}]" for k, why in killers))


# ---- planner --------------------------------------------------------------------------------------------------------------------------
def _groups(Ms, K, N, ldas=None, epi=gr.EPI_BF16):
    from fluxmi import ops

    out = []
    for i, M in enumerate(Ms):  # pointers are never followed by the planner: any non-NULL value
        kw = dict(gate=0x1000, resid=0x1000, ldr=N) if epi == gr.EPI_GATE_RESID else {}
        out.append(ops.make_group(0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, M, ldas[i] if ldas else K, N, **kw))
    return out


@pytest.mark.parametrize("Ms", [(4096, 512), (4608, 4608), (2304, 512, 77)])
@pytest.mark.parametrize("epi", [gr.EPI_BF16, gr.EPI_GATE_RESID])
def test_planner_keeps_mixed_lda_off_the_persistent_kernel(Ms, epi):
    """multi-round fp8 launches go to the persistent kernel (config 18 / 19), which has ONE lda for all its groups"""
    from fluxmi import ops

    N, K = 9216, 3072
    same = ops.gemm_plan(_groups(Ms, K, N, epi=epi), N, K, True, gr.E5M2, epi)
    assert any(l["cfg"] in (18, 19) for l in same), f"the anchor no longer plans a persistent launch: {same}"
    mixed = ops.gemm_plan(_groups(Ms, K, N, ldas=[K + 128 + 64 * i for i in range(len(Ms))], epi=epi), N, K, True, gr.E5M2, epi)
    for l in mixed:
        if l["cfg"] in (18, 19):
            assert len({K + 128 + 64 * i for i in l["groups"]}) == 1, f"groups with different lda on the persistent kernel: {mixed}"


@pytest.mark.parametrize("is_fp8,N,K,Ms", [(True, 9216, 3072, (4096, 512)), (True, 3072, 12288, (2304, 512)), (True, 256, 512, (257, 77)),
                                           (False, 3072, 15360, (512,)), (False, 256, 256, (255, 1)), (True, 3072, 3072, (4096, 512, 77))])
def test_planner_an_empty_group_changes_no_other_launch(is_fp8, N, K, Ms):
    from fluxmi import ops

    def launches(ms):
        plan = ops.gemm_plan(_groups(ms, K, N), N, K, is_fp8, gr.E5M2, gr.EPI_BF16)
        assert sorted(i for l in plan for i in l["groups"]) == list(range(len(ms)))
        return sorted((l["kind"], l["cfg"], l["S"], tuple(sorted(ms[i] for i in l["groups"] if ms[i]))) for l in plan if any(ms[i] for i in l["groups"]))

    base = launches(list(Ms))
    for pos in range(len(Ms) + 1):
        ms = list(Ms[:pos]) + [0] + list(Ms[pos:])
        assert launches(ms) == base, f"an empty group at position {pos} changes the plan of {Ms}"


# ---- the alignment contract of fluxmi_gemm_group_t -----------------------------------------------------------------------------------------
def _grouped(g, N, K, is_fp8, epi, cfg):
    from fluxmi import _lib

    arr = (_lib.GemmGroup * 1)(g)
    _lib.call("fluxmi_gemm_grouped", arr, 1, N, K, int(is_fp8), gr.E5M2, epi, cfg, None)


@pytest.mark.parametrize("field,value,is_fp8,epi", [
    ("A", 0x10008, True, gr.EPI_BF16), ("W", 0x10004, True, gr.EPI_BF16), ("lda", 520, True, gr.EPI_BF16), ("lda", 516, False, gr.EPI_BF16),
    ("C", 0x10008, True, gr.EPI_BF16), ("ldc", 260, True, gr.EPI_BF16), ("bias", 0x10008, False, gr.EPI_BF16),
    ("gate", 0x10008, True, gr.EPI_GATE_RESID), ("resid", 0x10002, True, gr.EPI_GATE_RESID), ("ldr", 257, True, gr.EPI_GATE_RESID),
    ("C2", 0x10008, True, gr.EPI_SPLIT), ("ldc2", 200, True, gr.EPI_SPLIT), ("c2_col0", 8, True, gr.EPI_SPLIT), ("split_n", 136, True, gr.EPI_SPLIT)])
def test_gemm_grouped_refuses_misaligned_views_by_name(field, value, is_fp8, epi):
    """the pointers are never followed: the refusal comes before any launch (no GPU here)"""
    from fluxmi import ops

    N, K = 256, 512
    kw = dict(A=0x10000, W=0x20000, bias=0x30000, sa_recip=0x40000, sb_recip=0x40010, Cout=0x50000, M=64, lda=K + 128, ldc=N + 128,
              gate=0x60000, resid=0x70000, ldr=N + 64, C2=0x80000, ldc2=384, split_n=128, c2_col0=128)
    kw[{"C": "Cout"}.get(field, field)] = value
    g = ops.make_group(kw.pop("A"), kw.pop("W"), kw.pop("bias"), kw.pop("sa_recip"), kw.pop("sb_recip"), kw.pop("Cout"), kw.pop("M"), kw.pop("lda"),
                       kw.pop("ldc"), **kw)
    with pytest.raises(RuntimeError, match=rf"group 0: {field}="):
        _grouped(g, N, K, is_fp8, epi, 13)


def test_gemm_grouped_alignment_is_what_the_kernels_need_and_no_more():
    """Where only the generic kernel can run (an N no tile divides) the outputs are stored one element at a time and their alignment is not
    looked at: the call gets past the check and is refused by the tile launcher instead (still host code).  Empty groups are not looked at."""
    from fluxmi import ops

    g = ops.make_group(0x10000, 0x20000, None, None, None, 0x50002, 64, 512, 259)
    with pytest.raises(RuntimeError, match="not tileable"):
        _grouped(g, 200, 512, True, gr.EPI_BF16, 13)
    g = ops.make_group(0x10008, 0x20004, None, None, None, 0x50002, 0, 513, 259)
    _grouped(g, 256, 512, True, gr.EPI_BF16, 100)  # M = 0: nothing to align, nothing launched
