"""GPU: every GEMM launcher on strided views inside sentinel frames, against fp64 (cases, frames and gates: tests/gemm_refs.py, shown to
reject wrong kernels by tests/test_gemm_refs_cpu.py).

Per case: (1) the C view is within the project's gate of the fp64 reference on the identical quantised operands -- assert_close_mag(mag =
accum_noise, ulps=1.05, min_exact=0.98), gate*y+x ulps=2.05, min_exact=0.95, cases of fewer than 4096 outputs pooled over fresh seeds;
(2) every sentinel of every frame is unchanged bit for bit: the rows from M to the end of a frame 256 rows taller than the tiles, the
columns left and right of the view, other groups' frames, the frame of a group of no rows, the separate residual buffer; (3) the same
launch on dense buffers gives the same bytes (the K loop does not depend on strides).  The split's bf16 half meets fp64; its fp8 half is
compared with the dense launch only (placement: its arithmetic is test_ops_gpu.py::test_quantising_epilogue_computed_vs_table_exhaustive's).
Each test prints its worst err / tol and its bit-exact share."""
import ctypes as C

import pytest
import torch

import gemm_refs as gr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(dev):
    from fluxmi import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def table(ops, dev):
    """(q_scale, 64 KiB GELU -> fp8 table) of the split epilogue"""
    qs = torch.tensor(41.0, device=dev)
    return qs, ops.build_quant_lut(qs, gr.E5M2, act=1)


def launch(ops, dev, case, prob, frames, table, cfg=None):
    groups, keep = [], []
    eb = 1 if case.op == "f8" else 2
    for p, f in zip(prob, frames):
        d = {k: p[k].to(dev) for k in ("w", "bias", "gate", "sar", "sbr") if p[k] is not None}
        keep.append(d)
        ptr = lambda k: d[k].data_ptr() if k in d else None  # noqa: E731
        kw = {}
        if case.epi == "gate":
            rb = f["r_buf"] if f["r_buf"] is not None else f["c_buf"]
            kw = dict(gate=ptr("gate"), resid=rb.data_ptr() + f["r_off"] * 2, ldr=f["ldr"])
        if case.epi == "split":
            kw = dict(C2=f["c2_buf"].data_ptr(), ldc2=f["ldc2"], split_n=case.split_n, c2_col0=f["c2_col0"], q_scale=table[0].data_ptr(), q_lut=table[1].data_ptr())
        groups.append(ops.make_group(f["a_buf"].data_ptr() + f["a_off"] * eb, ptr("w"), ptr("bias"), ptr("sar"), ptr("sbr"),
                                     f["c_buf"].data_ptr() + f["c_off"] * 2, f["M"], f["lda"], f["ldc"], **kw))
    ops.gemm_grouped(groups, case.N, case.K, case.op == "f8", case.fmt, gr.EPI_ID[case.epi], case.cfg if cfg is None else cfg)
    torch.cuda.synchronize()


def strided_and_dense(ops, dev, table, cfg=None, **frame_kw):
    """the launch callback of gr.run_case: the strided launch into `frames`, then the same launch on dense buffers, byte for byte"""
    def run(case, prob, frames, rep):
        if frame_kw:  # another geometry of the C view: rebuild the frames in place
            frames[:] = gr.make_frames(case, prob, dev, **frame_kw)
        launch(ops, dev, case, prob, frames, table, cfg)
        dense = gr.make_frames(case, prob, dev, dense=True)
        launch(ops, dev, case, prob, dense, table, cfg)
        bad = []
        for gi, (f, fd) in enumerate(zip(frames, dense)):
            if not torch.equal(gr.view_c(case, f).view(torch.int16), gr.view_c(case, fd).view(torch.int16)):
                bad.append(f"group {gi}: the strided launch differs from the dense launch")
            if case.epi == "split" and not torch.equal(gr.view_c2(case, f), gr.view_c2(case, fd)):
                bad.append(f"group {gi}: the fp8 half of the strided launch differs from the dense launch")
        return bad
    return run


@pytest.mark.parametrize("case", gr.CASES, ids=gr.CASE_IDS)
def test_gemm_on_strided_views(ops, dev, table, case):
    gr.run_case(case, strided_and_dense(ops, dev, table), device=dev)


@pytest.mark.parametrize("cfg", [gr.GENERIC, gr.AUTO], ids=["generic", "auto"])
@pytest.mark.parametrize("op,epi", [("f8", "plain"), ("bf16", "gate")])
def test_generic_kernel_takes_element_aligned_outputs(ops, dev, table, cfg, op, epi):
    """What include/fluxmi.h promises where only the generic kernel can run (N = 200: no tile divides it): C and resid one element at a
    time -- the view starts at column 3 of rows of N + 5 elements (2-byte alignment), the residual in place"""
    case = gr._case("odd", cfg, op, epi, [77, 1], 200, 512, bias=(1, 0), lda_extra=(0, 64), resid="inplace" if epi == "gate" else None)
    gr.run_case(case, strided_and_dense(ops, dev, table, c_off=3, c_pad=5), device=dev)


@pytest.mark.parametrize("epi", ["plain", "gate"])
def test_f8_gemm_entry_as_documented(dev, epi):
    """fluxmi_f8_gemm, the documented integration entry, called exactly as shown there: an own ctypes handle, the argtypes
    of the document, data_ptr() arguments, tile_cfg = -1 on the current stream -- against the same fp64 reference and gate"""
    from fluxmi import _lib

    lib = C.CDLL(_lib.LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int
    lib.fluxmi_last_error.restype = C.c_char_p
    lib.fluxmi_f8_gemm.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, i32, vp]
    case = gr._case("entry", gr.AUTO, "f8", epi, [300], 512, 768, resid="sep")
    p = gr.make_problem(case)[0]
    d = {k: p[k].to(dev) for k in ("a", "w", "bias", "gate", "x", "sar", "sbr") if p[k] is not None}
    out = torch.full((300, 512), float("nan"), dtype=torch.bfloat16, device=dev)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.fluxmi_f8_gemm(d["a"].data_ptr(), d["w"].data_ptr(), d["sar"].data_ptr(), d["sbr"].data_ptr(), d["bias"].data_ptr(), out.data_ptr(),
                            300, 512, 768, gr.E5M2, gr.EPI_ID[epi], d["gate"].data_ptr() if epi == "gate" else None,
                            d["x"].data_ptr() if epi == "gate" else None, None, -1, s)
    assert rc == 0, lib.fluxmi_last_error().decode()
    torch.cuda.synchronize()
    g = gr.gate_of(case)
    worst, exact = gr.stats(out.cpu().reshape(-1), p["ref"].reshape(-1), p["mag"].reshape(-1), g["ulps"])
    print(f"fluxmi_f8_gemm {epi}: worst err/tol {worst:.3f}, bit-exact {exact:.5f}")
    gr.assert_close_mag(out, p["ref"], mag=p["mag"], what=f"fluxmi_f8_gemm {epi}", **g)
