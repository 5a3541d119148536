"""CPU companion of tests/test_vae_kernels_gpu.py: proves the references, gates and case tables of tests/vae_refs.py.

  * the patch matrix written as index arithmetic equals the F.unfold construction of test_im2col3x3 in all three modes, and the unrounded
    convolution reference equals fp64 F.conv2d;
  * a torch fp32 matmul on the patch matrix, rounded at the kernel's rounding points, passes both gates at every case: the caps (0.99 / 0.95
    bit-exact) are attainable by a correct fp32 kernel;
  * every mutant of vae_refs.MUTANTS is rejected at every case where it changes anything, and by at least one case;
  * the call recorder, driven through the autoencoder's stage methods with fp32 emulations of the six ops, sees exactly EXPECTED_ARMS and
    every record passes check_call.
"""
import pytest
import torch
import torch.nn.functional as F

import vae_refs as vr
from helper_refs import bits

CPU_IM2COL_CASES = vr.IM2COL_CASES[:-1]  # the last one is the 4.3 GB second-trip case (GPU only)


def emul_run(x, w2, bias, gate, resid, mode):
    return vr.emul_conv3x3(x, w2, bias, mode, resid=resid, gate=gate).reshape(-1, w2.shape[0])


# ---- the references ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CPU_IM2COL_CASES, ids=vr.case_id)
def test_patch_matrix_equals_unfold(case):
    B, Hi, Wi, C, mode = case
    x = torch.randn(B, Hi, Wi, C, generator=torch.Generator().manual_seed(vr.seed_of("im2col", case))).bfloat16()
    got = vr.patch_matrix64(x, mode)
    H, W = vr.out_hw(Hi, Wi, mode)
    assert got.shape == (B * H * W, 9 * C) and got.dtype == torch.float64
    assert torch.equal(got, vr.emul_im2col3x3(x, mode).double())


@pytest.mark.parametrize("case", vr.CONV_CASES, ids=vr.case_id)
def test_unrounded_reference_equals_fp64_conv2d(case):
    B, Hi, Wi, C, Cout, mode = case
    x, w2, bias, _, _ = vr.conv_inputs(case)
    got = vr.conv3x3_ref(x, w2, bias, mode, rounded=False)
    w = w2.double().view(Cout, 3, 3, C).permute(0, 3, 1, 2)
    xn = x.double().permute(0, 3, 1, 2)
    if mode == 2:
        xn = F.interpolate(xn, scale_factor=2.0, mode="nearest")
    t = F.conv2d(F.pad(xn, (0, 1, 0, 1)), w, bias.double(), stride=2) if mode == -2 else F.conv2d(xn, w, bias.double(), padding=1)
    t = t.permute(0, 2, 3, 1).reshape(-1, Cout)
    assert got.shape == t.shape
    assert float((got - t).abs().max()) <= 1e-12 * float(t.abs().max())


def test_tables_reach_what_they_claim():
    for B, Hi, Wi, C, Cout, mode in vr.CONV_CASES:
        H, W = vr.out_hw(Hi, Wi, mode)
        assert C % 64 == 0 and Cout % 128 == 0 and (B * H * W) % vr.TILE_M, "every case is one the implicit kernel takes, with a ragged last tile"
        assert vr.conv_reps(B * H * W, Cout) * B * H * W * Cout >= 400
    assert len(vr.STRADDLING_CASES) >= 3
    for B, Hi, Wi, _, _, mode in vr.STRADDLING_CASES:  # some tile holds rows of two images
        H, W = vr.out_hw(Hi, Wi, mode)
        assert any((t * vr.TILE_M) // (H * W) != min(B * H * W - 1, t * vr.TILE_M + vr.TILE_M - 1) // (H * W) for t in range(-(-B * H * W // vr.TILE_M)))
    assert any(C == 192 for _, _, _, C, _, _ in vr.CONV_CASES) and {m for *_, m in vr.CONV_CASES} == {1, 2, -2}
    # exactly one im2col case passes the launch's thread count, and it also passes 2^31 elements
    assert [vr.im2col_vectors(*c) > vr.GRID1D_THREADS for c in vr.IM2COL_CASES] == [False] * len(CPU_IM2COL_CASES) + [True]
    assert vr.im2col_vectors(*vr.IM2COL_BIG) * 8 > 2 ** 31 and vr.im2col_vectors(*vr.IM2COL_BIG) < 2 * vr.GRID1D_THREADS


# ---- the gates are attainable in fp32 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", vr.EPILOGUES)
@pytest.mark.parametrize("case", vr.CONV_CASES, ids=vr.case_id)
def test_fp32_emulation_passes_the_gate(case, epi):
    ex, worst = vr.gate_conv_case(case, epi, emul_run, f"fp32 emulation {vr.case_id(case)} {epi}")
    print(f"fp32 emulation {vr.case_id(case)} {epi}: worst err/tol {worst:.3f} (<= 1), bit-exact {ex:.5f}")
    (x, w2, bias, gate, resid), ref, (mag, ulps, min_exact) = vr.conv_case_ref(case, epi)
    vr.gate_gemm(ref, ref, mag, ulps, min_exact, "the reference itself")


# ---- the gates reject wrong kernels --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mut", list(vr.MUTANTS))
def test_gate_rejects_mutant(mut):
    epis = ("resid",) if mut in ("gate_ones", "resid_prev_pixel") else vr.EPILOGUES
    rejected_at = []
    for case in vr.CONV_CASES:
        for epi in epis:
            _, ref, (mag, ulps, min_exact) = vr.conv_case_ref(case, epi)
            _, got, _ = vr.conv_case_ref(case, epi, mut=mut)
            if torch.equal(bits(got), bits(ref)):
                continue  # the slip changes nothing here (no such tap / block / tile in this case)
            with pytest.raises(AssertionError):
                vr.gate_gemm(got, ref, mag, ulps, min_exact, f"{mut} at {vr.case_id(case)} {epi}")
            rejected_at.append(f"{vr.case_id(case)}/{epi}")
    print(f"{mut} ({vr.MUTANTS[mut]}): rejected at {', '.join(rejected_at)}")
    assert rejected_at, f"no case of CONV_CASES rejects {mut}: the table is too weak"


def test_mutants_are_seen_where_they_are_aimed():
    """the case each slip was put into the table for"""
    aimed = {"sym_pad_stride2": (2, 18, 26, 64, 384, -2), "up_src_plus1": (2, 5, 7, 192, 128, 2), "base_of_first_row": (2, 9, 13, 128, 256, 1),
             "wrap_x": (2, 200, 1, 64, 128, 1), "taps_transposed": (1, 1, 200, 64, 128, 1), "cblock_reversed": (1, 3, 130, 512, 128, 1),
             "gate_ones": (3, 5, 7, 64, 128, 1), "resid_prev_pixel": (1, 1, 1, 128, 128, 2), "drop_last_tile_row": (1, 1, 1, 64, 128, 1)}
    assert set(aimed) == set(vr.MUTANTS)
    for mut, case in aimed.items():
        _, ref, (mag, ulps, min_exact) = vr.conv_case_ref(case, "resid")
        _, got, _ = vr.conv_case_ref(case, "resid", mut=mut)
        with pytest.raises(AssertionError):
            vr.gate_gemm(got, ref, mag, ulps, min_exact, mut)


# ---- the recorder --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attention", ["gemm", "streaming"])
@pytest.mark.parametrize("direction", ["decode", "encode"])
def test_stage_walk_on_the_cpu(monkeypatch, direction, attention):
    from fluxmi import ops

    for name, fn in vr.EMULATIONS.items():
        monkeypatch.setattr(ops, name, fn)
    rec = vr.record_calls(monkeypatch)
    ae = vr.walk_autoencoder(attention)
    with torch.inference_mode():
        out = vr.walk_stages(ae, direction, vr.walk_input(direction))
    h, w = vr.WALK_LATENT
    assert out.shape == ((vr.WALK_B, 4 * h, 4 * w, 3) if direction == "decode" else (vr.WALK_B, h, w, 2 * vr.WALK_PARAMS["z_channels"]))
    vr.check_all(rec, f"cpu emulation {direction}/{attention}")
    assert rec.arms() == vr.EXPECTED_ARMS[(direction, attention)], (
        f"missing {sorted(vr.EXPECTED_ARMS[(direction, attention)] - rec.arms())}, unexpected {sorted(rec.arms() - vr.EXPECTED_ARMS[(direction, attention)])}")


def test_check_call_rejects_a_wrong_record(monkeypatch):
    """check_call is not a formality: a record whose output belongs to another call of the same shape fails"""
    from fluxmi import ops

    for name, fn in vr.EMULATIONS.items():
        monkeypatch.setattr(ops, name, fn)
    rec = vr.record_calls(monkeypatch)
    ae = vr.walk_autoencoder("gemm")
    with torch.inference_mode():
        vr.walk_stages(ae, "decode", vr.walk_input("decode"))
    for kind in ("conv3x3", "im2col3x3", "linear", "groupnorm", "softmax_rows"):
        r = dict(next(r for r in rec.records if r["kind"] == kind))
        r["out"] = torch.roll(r["out"].reshape(-1, r["out"].shape[-1]), 1, 0).reshape(r["out"].shape)  # every row one place down
        with pytest.raises(AssertionError):
            vr.check_call(r)
