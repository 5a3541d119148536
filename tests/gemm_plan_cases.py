"""The case grid of tests/test_gemm_plan_cpu.py: grouped-GEMM launches as the engine issues them (layout flags included), as plain data.

A case is a dict: name, groups (dicts: M and the flags that the dispatcher reads), N, K, is_fp8, act_fmt, epi, batch (what an engine
announces through fluxmi_gemm_set_batch) and tuning (fluxmi_tuning_t overrides).  tests/golden/gemm_plan_parent.json holds, per case name,
the launch list that the dispatcher of the commit BEFORE the planner existed issued for it (profiles/r07_gemm_plan_record.patch)."""
H, HM, HEADS = 3072, 12288, 24
EPI_BF16, EPI_GELU_QUANT, EPI_GATE_RESID, EPI_SPLIT = 0, 1, 2, 3
PTR = 0x10000  # any non-null address: the planner looks at whether a pointer is set, never through it

GEOMETRIES = {"dev1024": (4096, 512), "dev768": (2304, 512), "ragged3257": (2745, 512), "schnell256": (256, 256)}  # name -> (Li, Lt)


def step_launches(Li, Lt, samples, fp8):
    """The six grouped Linear launches of one step (bench.py::gemm_shapes) for `samples` batch elements, with the flags of engine.hip: fused mode
    (fp8: row-pair weights and activations, quantising tables, V^T / K outputs on qkv and linear1) or the unfused bf16 flow (plain epilogues)."""
    L = Li + Lt
    Lp = (L + 63) // 64 * 64
    ap = int(fp8 and L % 2 == 0 and Lt % 2 == 0)
    fuse = fp8 and Lt % 16 == 0 and L >= 2048
    out = []

    def double(name, N, K, epi, **flags):
        gs = []
        for _ in range(samples):
            for st, M in enumerate((Lt, Li)):
                g = dict(M=M, lda=K, a_pairs=ap, **flags)
                if flags.get("fused"):
                    g.update(tok0=(0, Lt)[st], vt_rows=(Lt, Lp - Lt)[st], k_rows=L, vt_ld=Lp)
                gs.append(g)
        out.append((name, gs, N, K, epi))

    def single(name, N, K, epi, **flags):
        gs = []
        for _ in range(samples):
            g = dict(M=L, lda=K, a_pairs=ap, **flags)
            if flags.get("fused"):
                g.update(tok0=0, vt_rows=Lp, k_rows=L, vt_ld=Lp)
            gs.append(g)
        out.append((name, gs, N, K, epi))

    if fp8:
        double("qkv", 3 * H, H, EPI_BF16, W_pairs=1, fused=int(fuse))
        double("proj", H, H, EPI_GATE_RESID)
        double("mlp0", HM, H, EPI_GELU_QUANT, W_pairs=1, c8_pairs=ap, q_lut=1)
        double("mlp2", H, HM, EPI_GATE_RESID, W_pairs=1)
        single("linear1", 3 * H + HM, H, EPI_SPLIT, W_pairs=1, c8_pairs=ap, q_lut=1, split_n=3 * H, fused=int(fuse))
        single("linear2", H, H + HM, EPI_GATE_RESID, W_pairs=1)
    else:
        double("qkv", 3 * H, H, EPI_BF16)
        double("proj", H, H, EPI_GATE_RESID)
        double("mlp0", HM, H, EPI_BF16)
        double("mlp2", H, HM, EPI_GATE_RESID)
        single("linear1", 3 * H + HM, H, EPI_BF16)
        single("linear2", H, H + HM, EPI_GATE_RESID)
    return out


KNOB_VALUES = [("gemm_hybrid", 0), ("gemm_persist", 0), ("gemm_persist", 2), ("gemm_splitk", 0), ("gemm_tile192", 0), ("gemm_tile192", 2)] + \
              [("gemm_cfg", c) for c in (2, 13, 15, 16, 17, 18, 19, 20, 21)]


def cases():
    cs = []

    def add(name, groups, N, K, is_fp8, epi, batch=1, tuning=None):
        cs.append(dict(name=name, groups=groups, N=N, K=K, is_fp8=int(is_fp8), act_fmt=1, epi=epi, batch=batch, tuning=dict(tuning or {})))

    for geo, (Li, Lt) in GEOMETRIES.items():
        for name, gs, N, K, epi in step_launches(Li, Lt, 1, True):
            add(f"fp8/{geo}/{name}", gs, N, K, True, epi)
        for B in (1, 2, 4):  # bf16: the engine announces its batch and the dispatcher replays one sample's decisions
            for name, gs, N, K, epi in step_launches(Li, Lt, B, False):
                add(f"bf16/{geo}/B{B}/{name}", gs, N, K, False, epi, batch=B)
        # groups that do not divide by the announced batch: the whole-launch decision
        for name, gs, N, K, epi in step_launches(Li, Lt, 2, False):
            add(f"bf16/{geo}/B4_two_samples/{name}", gs, N, K, False, epi, batch=4)
    for name, gs, N, K, epi in step_launches(4096, 512, 2, True):
        add(f"fp8/dev1024/two_samples/{name}", gs, N, K, True, epi)
    for geo in ("dev1024", "dev768"):
        for knob, v in KNOB_VALUES:
            for name, gs, N, K, epi in step_launches(*GEOMETRIES[geo], 1, True):
                add(f"fp8/{geo}/{knob}={v}/{name}", gs, N, K, True, epi, tuning={knob: v})
    for knob, v in (("gemm_splitk", 0), ("gemm_hybrid", 0), ("gemm_tile192", 0), ("gemm_cfg", 13), ("gemm_cfg", 2)):
        for name, gs, N, K, epi in step_launches(256, 256, 1, False):
            add(f"bf16/schnell256/{knob}={v}/{name}", gs, N, K, False, epi, tuning={knob: v})
    one = lambda M, K: [dict(M=M, lda=K)]
    add("bf16/text_M512_K15360_splitk", one(512, 15360), H, 15360, False, EPI_BF16)
    add("bf16/text_M512_K15360_gate_resid", one(512, 15360), H, 15360, False, EPI_GATE_RESID)
    add("bf16/M512_N21504_cfg17", one(512, H), 21504, H, False, EPI_BF16)
    add("bf16/M512_N21504_gelu_quant", one(512, H), 21504, H, False, EPI_GELU_QUANT)
    add("fp8/20_groups_chunked", [dict(M=256 + 32 * (i % 3), lda=H) for i in range(20)], H, H, True, EPI_GATE_RESID)
    add("bf16/20_groups_chunked", [dict(M=512, lda=H) for _ in range(20)], H, H, False, EPI_BF16)
    add("bf16/40_groups_B2_chunked", [dict(M=(256, 1024)[i % 2], lda=H) for i in range(40)], H, H, False, EPI_BF16, batch=2)
    add("bf16/splitk_B8_piecewise_scratch", [dict(M=512, lda=15360) for _ in range(8)], H, 15360, False, EPI_BF16, batch=8)
    add("bf16/splitk_B4_one_group_whole_batch", one(2048, 15360), H, 15360, False, EPI_BF16, batch=4)
    add("bf16/splitk_B3_rows_do_not_divide", one(2048, 15360), H, 15360, False, EPI_BF16, batch=3)
    add("fp8/K64_N3072", one(4096, 64), H, 64, True, EPI_BF16)
    add("fp8/K48_generic", one(4096, 48), H, 48, True, EPI_BF16)
    add("fp8/K64_N200_generic", one(4096, 64), 200, 64, True, EPI_BF16)
    add("bf16/K64_img_in", one(4096, 64), H, 64, False, EPI_BF16)
    add("bf16/N64_final_layer", one(4096, H), 64, H, False, EPI_BF16)
    add("fp8/split_n_128_not_256", [dict(M=4608, lda=H, split_n=3 * H + 128)], 3 * H + HM, H, True, EPI_SPLIT)
    add("fp8/split_n_64_not_128", [dict(M=4608, lda=H, split_n=3 * H + 64)], 3 * H + HM, H, True, EPI_SPLIT)
    add("fp8/split_n_32_generic", [dict(M=512, lda=H, split_n=3 * H + 32)], 3 * H + HM, H, True, EPI_SPLIT)
    add("fp8/split_n_128_two_groups_peel", [dict(M=m, lda=H, split_n=3 * H + 128) for m in (512, 4096)], 3 * H + HM, H, True, EPI_SPLIT)
    assert len({c["name"] for c in cs}) == len(cs)
    return cs


def build_groups(GemmGroup, specs):
    """ctypes array of fluxmi_gemm_group_t for the group dicts of a case (fake, never dereferenced addresses)"""
    arr = (GemmGroup * len(specs))()
    for g, s in zip(arr, specs):
        g.A = g.W = g.C = PTR
        g.M, g.lda, g.ldc = s["M"], s["lda"], s["lda"]
        g.a_pairs, g.c8_pairs, g.split_n = s.get("a_pairs", 0), s.get("c8_pairs", 0), s.get("split_n", 0)
        g.W_pairs = PTR if s.get("W_pairs") else None
        g.q_lut = PTR if s.get("q_lut") else None
        if s.get("fused"):
            g.vt_out = g.k_out = g.pe = g.k_norm = PTR
            g.vt_ld, g.tok0, g.vt_rows, g.k_rows, g.kv_col0, g.heads, g.k_f16 = s["vt_ld"], s["tok0"], s["vt_rows"], s["k_rows"], H, HEADS, 1
    return arr
