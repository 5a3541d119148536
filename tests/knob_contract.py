"""What every value of every fluxmi_tuning_t knob (include/fluxmi.h) promises about the model's output -- ONE table that the CPU test
(test_abi_host_cpu.py::test_knob_contract_covers_every_tuning_field) checks against the library's validation and that the GPU sweeps
(test_tuning_knobs_gpu.py at hidden 256, test_full_geometry_gpu.py at hidden 3072) run value by value.

A contract is one of
  BIT          the latents / prediction are bit-identical to the defaults' (same kernels or kernels that compute the same bits);
  TOL(x)       within rel-L2 x of the defaults, and within the oracle tolerance the surrounding test already applies (the value changes
               the arithmetic: another summation order, another running-max grid, another K association);
  EXCLUDED     not run, with the reason (timing-only builds that are not meant to compute anything).
`with_` names knobs that are set together with the value (the comparison is still against the plain defaults).  A contract may differ
between the fp8 flow (F8Linear everywhere, fused step) and the bf16 flow (nn.Linear everywhere, Flux-schnell: unfused step, bf16
GEMMs with split-K and the bf16 tile choices): `per_flow(fp8=..., bf16=...)`.

The contracts are derived from the code, not from a run:
  * the fp8 tile configs share one MFMA shape and one K order, and since round 6 so do the bf16 ones;
  * split-K (bf16 operands only) associates K differently; a forced tile config or gemm_hybrid = 0 changes which launches split;
  * the persistent kernel's fused-K epilogue sums the QKNorm squares in another order than the one-tile-per-workgroup kernels' (<= 1 ulp
    of K, test_ops_gpu.py): fp8 values that take launches off the persistent kernel (a forced tile config, gemm_persist = 0, qlut = 0: the
    quantising launches qualify only with their table) run with fuse_kv = 1 (K by the relayout kernel, bit-identical to the default's
    fused K -- the fuse_kv = 1 entry below);
  * the balanced attention grid, the exact running max, other defer thresholds and a bf16 K all round P / O on another grid;
  * the one-wave-per-row LayerNorm reduces mean / variance in another order than the streaming kernel.
Tolerances: a change of the attention or LayerNorm arithmetic is re-gridded by every e5m2 quantisation behind it -- swapping the oracle's
own SDPA for an exact softmax moves its fp8 output by 3.5e-2 -- so the fp8 flow gets the engine-vs-oracle gate of
test_forward_matches_oracle_through_calibration (6e-2); the bf16 flow has no re-gridding and gets that test's bf16 gate (1e-2).
"""
from dataclasses import dataclass, field

FP8_TOL = 6e-2   # test_engine_gpu.py::test_forward_matches_oracle_through_calibration, fp8 models vs the fp8 oracle
BF16_TOL = 1e-2  # the same test, bf16 model vs the bf16 oracle


@dataclass(frozen=True)
class Contract:
    kind: str                 # "bit" | "tol" | "excluded"
    tol: float = 0.0          # rel-L2 bound of a "tol" contract
    reason: str = ""
    with_: tuple = field(default=())  # ((knob, value), ...) set together with the value under test

    @property
    def knobs_with(self):
        return dict(self.with_)


def BIT(reason="", **with_):
    return Contract("bit", 0.0, reason, tuple(sorted(with_.items())))


def TOL(x, reason, **with_):
    return Contract("tol", float(x), reason, tuple(sorted(with_.items())))


def EXCLUDED(reason):
    assert reason, "an excluded value needs its reason written down"
    return Contract("excluded", 0.0, reason)


def per_flow(fp8, bf16):
    return {"fp8": fp8, "bf16": bf16}


ATTN = "attention arithmetic on another grid (P / O rounding)"
SPLITK_OFF = "forcing a tile config switches the bf16 split-K choice off (split-K sums K in another association)"
# fp8 values that take launches off the persistent kernel (and with it its fused-K epilogue) run with K by the relayout kernel, see the module
# docstring; the bf16 flow never runs the persistent kernel (fp8 x e5m2 only) and takes config 13's fused K whatever these knobs say
_FORCED = dict(fuse_kv=1)


@dataclass(frozen=True)
class Knob:
    default: object
    lo: object                # validate() range (csrc/tuning.cpp); gemm_cfg: the accepted set is `values` itself
    hi: object
    values: dict              # value -> Contract or per_flow(...): every value validate() accepts (defaults included, contract BIT)
    doc: str = ""


def _gemm_cfg_values():
    v = {-1: BIT("default: cost model")}
    for cfg in (2, 13, 15, 16, 17, 20, 21):
        v[cfg] = per_flow(BIT("fp8 tile configs compute the same bits", **_FORCED), TOL(BF16_TOL, SPLITK_OFF))
    v[18] = per_flow(BIT("config 13 as a persistent kernel, taken where fluxmi_gemm_persist_ok holds", **_FORCED), TOL(BF16_TOL, SPLITK_OFF))
    v[19] = per_flow(BIT("timing build of config 18: the same arithmetic plus clock stamps (no debug buffer: none written)", **_FORCED),
                     TOL(BF16_TOL, SPLITK_OFF))
    return v


KNOBS = {
    "gemm_cfg": Knob(-1, -1, 21, _gemm_cfg_values(), "forced tile config where the launch supports it"),
    "gemm_splitk": Knob(1, 0, 1, {1: BIT(), 0: per_flow(BIT("split-K acts on bf16 operands only"), TOL(BF16_TOL, "one pass instead of split-K"))}),
    "gemm_hybrid": Knob(1, 0, 1, {1: BIT(), 0: per_flow(BIT("no 128x128 peel: the tile configs give the same bits"),
                                                          TOL(BF16_TOL, "the peel decides which groups split K"))}),
    "gemm_esel": Knob(1, 0, 1, {1: BIT(), 0: BIT("run-time epilogue switch: the same epilogue arithmetic")}),
    "gemm_persist": Knob(1, 0, 2, {1: BIT(), 0: per_flow(BIT("one tile per workgroup: same bits (fused K through the relayout kernel)", **_FORCED),
                                                          BIT("the persistent kernel takes fp8 operands only")),
                                   2: BIT("timing build of the persistent kernel: the same arithmetic plus clock stamps")}),
    "attn_var": Knob(0, 0, 3, {0: BIT(), 1: BIT("bit 0 selects nothing (reserved)"), 2: TOL(FP8_TOL, "exact running max: " + ATTN),
                               3: TOL(FP8_TOL, "exact running max: " + ATTN)}),
    # bit 1 (value 2) drops a barrier of the 8-wave kernel: a timing ablation whose results are not defined; bit 3 (8) stores the fp8
    # output as 16 x 4 B per lane (the same bytes); bits 0 and 2 select nothing
    "attn_abl": Knob(0, 0, 15, {v: (EXCLUDED("bit 1 removes a barrier of the 8-wave attention kernel: timing only, results undefined")
                                    if v & 2 else BIT("bit 3: 4-byte fp8 stores, the same bytes; bits 0 and 2 select nothing"))
                                for v in range(16)}),
    "attn_defer_log2": Knob(8.0, 0.0, 16.0, {8.0: BIT(), 0.0: TOL(FP8_TOL, "rescale at every growth: " + ATTN),
                                             4.0: TOL(FP8_TOL, "another rescale threshold: " + ATTN),
                                             16.0: TOL(FP8_TOL, "another rescale threshold: " + ATTN)}),
    "attn_f16k": Knob(1, 0, 1, {1: BIT(), 0: TOL(FP8_TOL, "K in bf16 and the unfolded arithmetic: " + ATTN)}),
    # fp8: the persistent kernel's fused K sums in the relayout kernel's order; bf16 operands take config 13's fused K (another order, 99.9 %
    # of the elements identical: engine.hip double_block)
    "fuse_kv": Knob(2, 0, 2, {2: BIT(), 1: per_flow(BIT("K by the relayout kernel, whose order the persistent fused-K tiles follow"),
                                                    TOL(BF16_TOL, "K by the relayout kernel instead of config 13's fused K")),
                              0: per_flow(BIT("K and V^T by the relayout kernel (V^T is a copy)"),
                                          TOL(BF16_TOL, "K by the relayout kernel instead of config 13's fused K"))}),
    # without the table the quantising launches (mlp.0, linear1) do not qualify for the persistent kernel (fluxmi_gemm_persist_ok)
    "qlut": Knob(1, 0, 1, {1: BIT(), 0: per_flow(BIT("arithmetic GELU -> fp8 epilogue: the table holds its results", **_FORCED),
                                                 BIT("the tables serve fused fp8 epilogues only"))}),
    "ln_variant": Knob(2, 1, 3, {2: BIT(), 3: BIT("the streaming kernel at two workgroups per CU: the same per-row arithmetic"),
                                 1: per_flow(TOL(FP8_TOL, "one wave per row: mean / variance reduced in another order"),
                                             TOL(BF16_TOL, "one wave per row: mean / variance reduced in another order"))}),
    "roctx": Knob(0, 0, 1, {0: BIT(), 1: BIT("profiler ranges on the host only")}),
    "prefetch": Knob(1, 0, 3, {1: BIT(), 0: BIT("no weight prefetch (extra workgroups only read)"), 2: BIT("prefetch of mlp.2 as well"),
                               3: BIT("prefetch of the next linear1 as well")}),
    "w_pairs": Knob(1, 0, 1, {1: BIT(), 0: BIT("the kernels read the plain weights: the same values")}),
    "log": Knob(0, 0, 1, {0: BIT(), 1: BIT("prints the struct to stderr")}),
    "gemm_tile192": Knob(1, 0, 2, {1: BIT(), 0: BIT("256-row tiles only: the same kernel, same bits"), 2: BIT("192-row tiles only: same bits")}),
    "attn_split": Knob(1, 0, 2, {1: BIT(), 0: TOL(FP8_TOL, "one workgroup per task where the default splits a thin last round: " + ATTN),
                                 2: TOL(FP8_TOL, "balanced grid wherever a plan exists: " + ATTN)}),
    "a_pairs": Knob(1, 0, 1, {1: BIT(), 0: BIT("plain activation rows: the same values")}),
}


def contract(knob, value, flow):
    """the Contract of `value` of `knob` in `flow` ("fp8" / "bf16"); a TOL of the fp8 flow becomes the bf16 gate in the bf16 flow unless
    the table says otherwise per flow"""
    c = KNOBS[knob].values[value]
    if isinstance(c, dict):
        return c[flow]
    if c.kind == "tol" and flow == "bf16":
        return Contract("tol", min(c.tol, BF16_TOL), c.reason, c.with_)
    return c


def sweep(flow):
    """(knob, value, contract) for every non-default value that is run (defaults and EXCLUDED values are not)"""
    out = []
    for name, k in KNOBS.items():
        for v in k.values:
            if v == k.default:
                continue
            c = contract(name, v, flow)
            if c.kind != "excluded":
                out.append((name, v, c))
    return out


def knobs_of(name, value, c):
    d = dict(c.knobs_with)
    d[name] = value
    return d
