"""The autoencoder's convolutions -- the implicit 3x3 GEMM (csrc/gemm.hip `CONV`, fluxmi_conv3x3), fluxmi_im2col3x3 and every launch of a
whole decode / encode -- against the fp64 references of tests/vae_refs.py, element by element.

The gates are the ones the first tests of the GEMM set (test_bf16_gemm, test_gemm_split_k); tests/test_vae_refs_cpu.py shows that each
rejects the wrong kernels it is meant to catch and that a torch fp32 matmul passes it at every case.  The kernels run on guarded buffers:
the input is a slice of a NaN-filled allocation (a tap that leaves the image without going through the zero page brings a NaN in), the
output and the residual are slices of sentinel-filled buffers with one whole tile behind row M, compared bit for bit afterwards.  Each test
prints its worst figure.
"""
import pytest
import torch

import vae_refs as vr
from helper_refs import bits, sentinel_like

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(dev):
    from fluxmi import ops as _ops

    return _ops


def assert_sentinel(t, what):
    assert bool((bits(t) == bits(sentinel_like((1,), t.device))).all()), f"{what}: a sentinel was overwritten"


def guarded_input(x, dev):
    """x [B, Hi, Wi, C] -> the same values as a slice of a NaN-filled allocation, (Wi + 2) * C elements of guard on each side"""
    B, Hi, Wi, C = x.shape
    guard = (Wi + 2) * C
    buf = torch.full((2 * guard + x.numel(),), float("nan"), dtype=torch.bfloat16, device=dev)
    buf[guard : guard + x.numel()] = x.to(dev).reshape(-1)
    return buf[guard : guard + x.numel()].view(B, Hi, Wi, C), buf


def framed_rows(M, N, dev, fill=None):
    """[M, N] rows inside a sentinel-filled [TILE_M + M + TILE_M, N] buffer: (view, buffer)"""
    buf = sentinel_like((2 * vr.TILE_M + M, N), dev)
    view = buf[vr.TILE_M : vr.TILE_M + M]
    if fill is not None:
        view.copy_(fill.to(dev).reshape(M, N))
    return view, buf


def assert_frame(buf, M, what):
    assert_sentinel(buf[: vr.TILE_M], f"{what}: rows before the view")
    assert_sentinel(buf[vr.TILE_M + M :], f"{what}: the tile of rows behind row M")


def run_conv(ops, dev, x, w2, bias, gate, resid, mode):
    """one fluxmi_conv3x3 launch on guarded buffers -> [M, Cout] on the host"""
    from fluxmi import _lib

    B, Hi, Wi, C = x.shape
    Cout = w2.shape[0]
    H, W = vr.out_hw(Hi, Wi, mode)
    M = B * H * W
    xv, xbuf = guarded_input(x, dev)
    out, obuf = framed_rows(M, Cout, dev)
    rv, rbuf = framed_rows(M, Cout, dev, resid) if resid is not None else (None, None)
    w2d, bd, gd = w2.to(dev), bias.to(dev), None if gate is None else gate.to(dev)
    _lib.call("fluxmi_conv3x3", ops._p(xv), ops._p(w2d), ops._p(bd), ops._p(gd), ops._p(rv), ops._p(out), B, H, W, C, Cout, mode, ops._stream())
    torch.cuda.synchronize()
    what = f"conv3x3 {tuple(x.shape)} -> {Cout} mode {mode}"
    assert_frame(obuf, M, f"{what}: out")
    if rbuf is not None:
        assert_frame(rbuf, M, f"{what}: resid")
        assert torch.equal(bits(rv), bits(resid.to(dev).reshape(M, Cout))), f"{what}: the residual was written"
    assert torch.equal(bits(xv), bits(x.to(dev))), f"{what}: the input was written"
    return out.cpu()


# ---- the implicit kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", vr.EPILOGUES)
@pytest.mark.parametrize("case", vr.CONV_CASES, ids=vr.case_id)
def test_conv3x3_against_fp64(ops, dev, case, epi):
    """Every element within the gate of its epilogue, no NaN (vr.gate_gemm asserts it), the rows behind M still the sentinel as bits"""
    what = f"conv3x3 {vr.case_id(case)} {epi}"
    ex, worst = vr.gate_conv_case(case, epi, lambda *a: run_conv(ops, dev, *a), what)
    print(f"{what}: worst err/tol {worst:.3f} (<= 1), bit-exact {ex:.5f} (>= {0.99 if epi == 'plain' else 0.95})")


@pytest.mark.parametrize("case", vr.STRADDLING_CASES, ids=vr.case_id)
def test_conv3x3_run_to_run_and_batch_alone(ops, dev, case):
    """Two launches give the same bits, and image b computed alone gives the bits it has inside the batch, where its rows share a tile
    with another image's: same kernel, same K order, one tile family."""
    B, Hi, Wi, C, Cout, mode = case
    hw = vr.out_hw(Hi, Wi, mode)[0] * vr.out_hw(Hi, Wi, mode)[1]
    x, w2, bias, gate, resid = vr.conv_inputs(case)
    for g, r in ((None, None), (gate, resid)):
        a = run_conv(ops, dev, x, w2, bias, g, r, mode)
        assert torch.equal(bits(a), bits(run_conv(ops, dev, x, w2, bias, g, r, mode))), f"{vr.case_id(case)}: two launches differ"
        for b in range(B):
            alone = run_conv(ops, dev, x[b : b + 1], w2, bias, g, None if r is None else r[b * hw : (b + 1) * hw], mode)
            assert torch.equal(bits(alone), bits(a[b * hw : (b + 1) * hw])), f"{vr.case_id(case)}: image {b} alone differs from image {b} inside B = {B}"


def test_conv3x3_wrapper_refusals(ops, dev):
    x = torch.zeros(1, 5, 6, 64, dtype=torch.bfloat16, device=dev)
    w2 = torch.zeros(128, 9 * 64, dtype=torch.bfloat16, device=dev)
    with pytest.raises(ValueError, match="even input dims"):
        ops.conv3x3(x, w2, None, -2)
    with pytest.raises(ValueError, match=r"needs w2 \[Cout, 9\*C\]"):
        ops.conv3x3(x, w2[:, : 9 * 64 - 64].contiguous(), None, 1)


# ---- im2col --------------------------------------------------------------------------------------------------------------------
def run_im2col(ops, dev, xv, mode):
    from fluxmi import _lib

    B, Hi, Wi, C = xv.shape
    H, W = vr.out_hw(Hi, Wi, mode)
    M = B * H * W
    col, cbuf = framed_rows(M, 9 * C, dev)  # filled from the sentinel: an unwritten vector shows
    _lib.call("fluxmi_im2col3x3", ops._p(xv), ops._p(col), B, H, W, C, mode, ops._stream())
    torch.cuda.synchronize()
    assert_frame(cbuf, M, f"im2col3x3 {tuple(xv.shape)} mode {mode}")
    return col


@pytest.mark.parametrize("case", vr.IM2COL_CASES[:-1], ids=vr.case_id)
def test_im2col3x3_against_definition(ops, dev, case):
    B, Hi, Wi, C, mode = case
    x = torch.randn(B, Hi, Wi, C, generator=torch.Generator().manual_seed(vr.seed_of("im2col", case))).bfloat16()
    xv, _ = guarded_input(x, dev)
    col = run_im2col(ops, dev, xv, mode).cpu()
    ref = vr.patch_matrix64(x, mode)
    assert col.shape == ref.shape and torch.equal(col.double(), ref) and torch.equal(bits(col), bits(vr.patch_rows(x, mode)))


def test_im2col3x3_second_trip_of_the_grid_stride_loop(ops, dev):
    """vr.IM2COL_BIG: 268 697 664 vectors for the 268 431 360 threads the launch gets, 2 149 581 312 > 2^31 elements of `col`.  The same
    index arithmetic (vr.patch_rows) evaluated on the device, a million rows at a time, bit for bit."""
    B, Hi, Wi, C, mode = vr.IM2COL_BIG
    assert vr.im2col_vectors(*vr.IM2COL_BIG) > vr.GRID1D_THREADS
    x = torch.randn(B, Hi, Wi, C, device=dev, generator=torch.Generator(device=dev).manual_seed(5)).bfloat16()
    xv, _ = guarded_input(x, dev)
    col = run_im2col(ops, dev, xv, mode)
    step = 1 << 20
    for r0 in range(0, col.shape[0], step):
        rows = torch.arange(r0, min(col.shape[0], r0 + step), device=dev)
        assert torch.equal(bits(col[r0 : r0 + step]), bits(vr.patch_rows(x, mode, rows))), f"rows {r0}..{r0 + step} of the patch matrix differ"


# ---- every launch of a decode / encode -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("attention", ["gemm", "streaming"])
@pytest.mark.parametrize("direction", ["decode", "encode"])
def test_autoencoder_stage_walk(dev, monkeypatch, direction, attention):
    """ch 64, ch_mult [1, 2, 8], B = 2 on a 5 x 6 latent: 30 / 120 / 480 pixels per image, so tiles straddle images at every resolution and
    the gemm attention runs zero-padded and -inf-masked.  Each launch is compared with its reference on the input it received, so no error
    accumulates and the kernels' own gates apply; the set of dispatch arms seen must be exactly vr.EXPECTED_ARMS."""
    rec = vr.record_calls(monkeypatch)
    ae = vr.walk_autoencoder(attention, dev)
    inp = vr.walk_input(direction).to(dev)
    out = ae.decode(inp) if direction == "decode" else ae.encode_moments(inp)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    vr.check_all(rec, f"walk {direction}/{attention}")
    want = vr.EXPECTED_ARMS[(direction, attention)]
    assert rec.arms() == want, f"missing {sorted(want - rec.arms())}, unexpected {sorted(rec.arms() - want)}"


@pytest.mark.parametrize("direction", ["decode", "encode"])
def test_implicit_conv_flag_keeps_every_bit(dev, monkeypatch, direction):
    """implicit_conv = False (im2col + GEMM for every 3x3 convolution) gives the bits of the default dispatch"""
    from fluxmi import ops as o

    ae = vr.walk_autoencoder("gemm", dev)
    inp = vr.walk_input(direction).to(dev)
    run = (lambda: ae.decode(inp)) if direction == "decode" else (lambda: ae.encode_moments(inp))
    a = run()
    ae.implicit_conv = False

    def boom(*a, **k):
        raise AssertionError("implicit_conv = False reached ops.conv3x3")

    monkeypatch.setattr(o, "conv3x3", boom)
    b = run()
    torch.cuda.synchronize()
    assert a.shape == b.shape and torch.equal(bits(a), bits(b)), f"{direction}: {int((bits(a) != bits(b)).sum())} of {a.numel()} values differ"
