"""CPU (no GPU): the GEMM launch planner (csrc/gemm_dispatch.cpp, exported as fluxmi_gemm_plan) decides what the dispatcher decided
before planning and launching were separated.

Every fp8 tile config gives the same bits and so does every one-pass bf16 config, so no output test can see a launch that went to the
wrong tile height or a peel that stopped happening; it shows as a few percent of step time.  The expected table
(tests/golden/gemm_plan_parent.json) was RECORDED from the dispatcher of the commit before the planner existed, with its four terminal
launch calls replaced by a recorder (profiles/r07_gemm_plan_record.patch) -- it is not an output of the planner under test."""
import json
import os

import pytest

import gemm_plan_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("tile", "generic", "splitk")
# tile config -> (bm, bn, K-step bytes, minimum K bytes), restated from csrc/gemm_cfg.h
TILES = {2: (128, 128, 128, 128), 13: (256, 256, 64, 64), 15: (128, 64, 128, 128), 16: (256, 256, 256, 256), 17: (192, 256, 256, 256),
         18: (256, 256, 256, 512), 19: (256, 256, 256, 512), 20: (224, 256, 256, 256), 21: (160, 256, 256, 256)}


@pytest.fixture(scope="module")
def plans():
    """{case name: (case, plan)} for the whole grid, planned once"""
    from fluxmi import _lib, ops

    out = {}
    for c in gc.cases():
        groups = gc.build_groups(_lib.GemmGroup, c["groups"])
        with _lib.tuning(**c["tuning"]):
            out[c["name"]] = (c, ops.gemm_plan(list(groups), c["N"], c["K"], c["is_fp8"], c["act_fmt"], c["epi"], batch=c["batch"]))
    return out


@pytest.fixture(scope="module")
def parent():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_plan_parent.json")))


def rows_of(case, launch):
    return [case["groups"][i]["M"] for i in launch["groups"]]


def test_plan_equals_the_recorded_dispatcher(plans, parent):
    """kind, tile config, split-K slices and the row counts of the groups of every launch, in launch order, for every case of the grid"""
    assert sorted(plans) == sorted(parent) and len(plans) >= 300
    bad = []
    for name, (case, plan) in plans.items():
        got = [[KINDS.index(l["kind"]), l["cfg"], l["S"], rows_of(case, l)] for l in plan]
        if got != parent[name]:
            bad.append((name, got, parent[name]))
    assert not bad, f"{len(bad)} of {len(plans)} plans differ from the recorded dispatcher; first: {bad[0]}"


def test_recorded_table_shows_the_documented_decisions(parent):
    """Anchors from the dispatcher's own comments: were they missing from the RECORDED table, the recording would be wrong."""
    tile = lambda cfg, *rows: [0, cfg, 0, list(rows)]
    assert parent["fp8/dev1024/mlp0"] == [tile(18, 512, 4096)]                        # 864 tiles leave 96 in the last round: no peel
    assert parent["fp8/dev768/mlp0"] == [tile(18, 2304), tile(2, 512)]                # 2 rounds + 16 tiles: the text stream is peeled
    assert parent["fp8/dev1024/linear2"] == [tile(20, 4608)]                          # 224-row tiles: 252 tiles, one round
    assert parent["fp8/dev768/mlp2"] == [tile(21, 512, 2304)] and parent["fp8/dev768/linear2"] == [tile(21, 2816)]
    assert parent["fp8/dev768/gemm_tile192=2/mlp2"] == [tile(17, 512, 2304)] and parent["fp8/dev768/gemm_tile192=2/linear2"] == [tile(17, 2816)]
    assert parent["bf16/text_M512_K15360_splitk"] == [[2, -1, 10, [512]]] and parent["bf16/M512_N21504_cfg17"] == [tile(17, 512)]
    assert parent["fp8/K48_generic"] == [[1, -1, 0, [4096]]]
    assert [len(l[3]) for l in parent["fp8/20_groups_chunked"]] == [16, 4]
    assert parent["bf16/splitk_B8_piecewise_scratch"] == [[2, -1, 10, [512] * 4]] * 2  # 8 x 512 rows x 10 slices exceed the 256 MiB scratch
    # every tile config, the generic kernel and split-K occur somewhere in the grid
    kinds = {(l[0], l[1]) for launches in parent.values() for l in launches}
    assert kinds == {(0, c) for c in TILES} | {(1, -1), (2, -1)}


def supports(case, launch):
    """fluxmi_gemm_cfg_supports, restated: tile config launch["cfg"] runs these groups as they stand"""
    cfg, gs = launch["cfg"], [case["groups"][i] for i in launch["groups"]]
    bm, bn, kstep, min_k = TILES[cfg]
    kb = case["K"] * (1 if case["is_fp8"] else 2)
    f8_gate = case["is_fp8"] and case["act_fmt"] == 1 and case["epi"] == gc.EPI_GATE_RESID
    bf_plain = not case["is_fp8"] and case["epi"] in (gc.EPI_BF16, gc.EPI_GATE_RESID)
    ok = case["N"] % bn == 0 and kb % kstep == 0 and kb >= min_k
    ok &= case["epi"] != gc.EPI_SPLIT or gs[0].get("split_n", 0) % bn == 0
    ok &= cfg in (13, 16, 18, 19) or not any(g.get("fused") for g in gs)
    if cfg in (18, 19):  # the persistent kernel: fp8 x e5m2, its four epilogues, the quantising ones through a table, one layout per launch
        ok &= bool(case["is_fp8"]) and case["epi"] in (gc.EPI_BF16, gc.EPI_GATE_RESID, gc.EPI_SPLIT, gc.EPI_GELU_QUANT)
        ok &= case["epi"] not in (gc.EPI_SPLIT, gc.EPI_GELU_QUANT) or all(g.get("q_lut") for g in gs)
        ok &= len({(g["lda"], bool(g.get("W_pairs")), bool(g.get("a_pairs"))) for g in gs}) == 1
    if cfg == 17:
        ok &= f8_gate or bf_plain
    if cfg in (20, 21):
        ok &= f8_gate
    return bool(ok)


def test_every_plan_is_a_partition_its_configs_can_run(plans):
    for name, (case, plan) in plans.items():
        assert sorted(i for l in plan for i in l["groups"]) == list(range(len(case["groups"]))), f"{name}: not a permutation of the groups"
        for l in plan:
            assert 1 <= len(l["groups"]) <= 16, name
            assert (l["kind"] == "tile") == (l["cfg"] >= 0) and (l["kind"] == "splitk") == (l["S"] >= 2), (name, l)
            if l["kind"] == "tile":
                assert supports(case, l), f"{name}: tile config {l['cfg']} does not run this launch"
            if l["kind"] == "splitk":  # bf16 only, partial tiles inside the scratch, never the row-pair layouts or fused outputs
                rows = sum((m + 255) // 256 * 256 for m in rows_of(case, l))
                assert not case["is_fp8"] and l["S"] * rows * case["N"] * 4 <= 256 << 20, (name, l)
                assert not any(g.get("fused") or g.get("a_pairs") or g.get("c8_pairs") for g in (case["groups"][i] for i in l["groups"]))


def test_plan_reports_errors_and_short_buffers():
    import ctypes as C

    from fluxmi import _lib

    g = gc.build_groups(_lib.GemmGroup, [dict(M=4608, lda=3072, fused=1, tok0=8, vt_rows=4608, k_rows=4608, vt_ld=4608)])
    n = C.c_int()
    buf = (C.c_int * 8)()
    assert _lib.lib.fluxmi_gemm_plan(g, 1, 9216, 3072, 1, 1, 0, 1, buf, 8, C.byref(n)) == 1 and b"tok0" in _lib.lib.fluxmi_last_error()
    g = gc.build_groups(_lib.GemmGroup, [dict(M=512, lda=3072)] * 2)
    assert _lib.lib.fluxmi_gemm_plan(g, 2, 3072, 3072, 1, 1, 0, 1, buf, 3, C.byref(n)) == 1 and n.value == 6
    assert _lib.lib.fluxmi_gemm_plan(g, 2, 3072, 3072, 1, 1, 0, 1, buf, 8, C.byref(n)) == 0 and list(buf[:6])[3:] == [2, 0, 1]
    assert _lib.lib.fluxmi_gemm_plan(g, 0, 3072, 3072, 1, 1, 0, 1, buf, 8, C.byref(n)) == 1
