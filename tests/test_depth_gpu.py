"""The Depth Anything estimator on the GPU (csrc/depth.hip, modules/depth.py) against tests/depth_ref.py.

Kernels, against fp64 on the bf16 input values.  The per-element gate has the form of the attention tests' (tests/attention_ref.py):
    |got - ref| <= MARGIN * (u * |ref| + n * 2^-24 * A),   MARGIN = 1.25, u = 2^-8 (one bf16 rounding, to nearest)
where A is the sum of the absolute values the fp32 chain adds up and n counts the fp32 roundings on the longest path to the output:
  unary gelu   A = 0.5 |x| (1 + |erf(x / sqrt 2)|), n = 8: the argument's product and erf's own error (<= 4 ulp) reach 1 + erf as at most
               7 * 2^-24 absolutely, which 0.5 |x| scales; two more products follow.  ReLU is exact.
  resize       A = sum of |weight * tap| over the four taps, n = 8: 1 - l, a product and a sum per axis (6), the source coordinate being
               the reference's own fp32 value; 2 spare.  With `add` the bf16 rounding of the resized value comes on top: + u * |v|.
  depth_head   A = sum |x_c w_c| + |bias|, n = C + 1, no bf16 rounding at all (the output is fp32).
The stride-2 convolution is held to the VAE convolution tests' gate (tests/vae_refs.py); the depth map byte for byte to the reference except
within 2^-10 of a rounding step (the blur test's rule), at most 1 % of the pixels.  Operands are channel windows of sentinel-filled buffers,
the frame around every output must stay intact, results must be bit-equal run to run and alone versus in a batch.

Model: the native backbone features and depth against the fp64 reference at the four grids, B = 1 and 3: rel-L2 <= 1.5 x that of the
reference with bf16 rounding at the native rounding points (the margin of the CLIP tower's test in tests/test_ip_adapter_gpu.py).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import depth_ref as dr
import helper_refs as hr
import vae_refs as vr
from helper_refs import bits, sentinel_like

pytestmark = pytest.mark.gpu

MARGIN, U = 1.25, 2.0 ** -8
SIZES = [((1, 1), (1, 1)), ((1, 1), (4, 4)), ((2, 2), (3, 3)), ((19, 19), (37, 37)), ((5, 5), (5, 5)), ((2, 3), (3, 5)), ((4, 7), (1, 9)), ((3, 1), (6, 2))]
CHANNELS = [8, 64, 136]


@pytest.fixture(scope="module")
def ops():
    from fluxmi import ops as o

    return o


def window(dev, shape, lead, trail, data=None):
    """a bf16 [..., C] window `lead` channels inside a sentinel-filled [..., lead + C + trail] buffer -> (buffer, window view)"""
    buf = sentinel_like(tuple(shape[:-1]) + (lead + shape[-1] + trail,), dev)
    win = buf[..., lead:lead + shape[-1]]
    if data is not None:
        win.copy_(data.to(dev))
    return buf, win


def frame_intact(buf, lead, C):
    full = buf.cpu()
    return bool((bits(full[..., :lead]) == hr.SENTINEL).all() and (bits(full[..., lead + C:]) == hr.SENTINEL).all())


def gate(got, ref, A, n, what, extra=None):
    """the module docstring's per-element gate; returns the worst err / bound"""
    got, ref = got.detach().cpu().double(), ref.double()
    assert torch.isfinite(got).all(), f"{what}: non-finite outputs"
    bound = MARGIN * (U * ref.abs() + n * 2.0 ** -24 * A + (0 if extra is None else extra))
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    assert bool((err <= bound).all()), f"{what}: worst err / bound {worst:.2f} at {int((err > bound).sum())} elements"
    return worst


# ---- fluxmi_unary ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("cols", CHANNELS + [1, 13])
def test_unary_against_fp64(ops, dev, cols, B):
    g = torch.Generator().manual_seed(hr.seed_of("unary", cols, B))
    rows = 37
    x = (3.0 * torch.randn(B, rows, cols, generator=g)).bfloat16()
    x[0, 0, 0], x[0, 1, 0], x[0, 2, 0] = 0.0, -9.5, 30.0
    x64 = x.double()
    erf = torch.erf(x64 / math.sqrt(2.0))
    refs = {"gelu": 0.5 * x64 * (1 + erf), "relu": torch.relu(x64)}
    for kind in ("gelu", "relu"):
        A = 0.5 * x64.abs() * (1 + erf.abs()) if kind == "gelu" else torch.zeros_like(x64)
        dense = ops.unary(x.to(dev), kind)
        w = gate(dense, refs[kind], A, 8, f"unary {kind} cols={cols} B={B}")
        if kind == "relu":
            assert torch.equal(dense.cpu(), torch.relu(x)), "ReLU must be exact"
        # column windows of wider sentinel buffers: an aligned one (lead 8, stride % 8 == 0) and one that is not (lead 3, odd stride)
        for lead, trail in ((8, 8 + (-cols) % 8), (3, 2 + cols % 2)):
            ibuf, iwin = window(dev, x.shape, lead, trail, x)
            obuf, owin = window(dev, x.shape, lead, trail)
            assert ops.unary(iwin, kind, out=owin).data_ptr() == owin.data_ptr()
            assert torch.equal(bits(owin.cpu()), bits(dense.cpu())), (kind, lead, "a strided run differs from the dense one")
            assert frame_intact(obuf, lead, cols) and frame_intact(ibuf, lead, cols), (kind, lead)
        assert torch.equal(bits(ops.unary(x.to(dev), kind)), bits(dense)), "two runs differ"
        alone = ops.unary(x[B - 1:].to(dev), kind)
        assert torch.equal(bits(alone[0]), bits(dense[B - 1])), "a sample alone differs from the same sample in a batch"
        inplace = x.to(dev).clone()
        ops.unary(inplace, kind, out=inplace)
        assert torch.equal(bits(inplace), bits(dense)), "in place differs"
        print(f"unary {kind} cols={cols} B={B}: worst err / bound {w:.3f}")


def test_unary_gelu_over_the_normal_range_of_bf16(ops, dev):
    """every bf16 value with 1e-30 < |x| < 1e30, and zero (subnormal fp32 intermediates are left out: whether they are kept is the
    device's denormal mode, not this kernel's arithmetic)"""
    x = hr.all_finite_bf16()
    x = x[(x.abs() < 1e30) & ((x.abs() > 1e-30) | (x == 0))].reshape(1, -1)
    x64 = x.double()
    erf = torch.erf(x64 / math.sqrt(2.0))
    got = ops.unary(x.to(dev), "gelu")
    gate(got, 0.5 * x64 * (1 + erf), 0.5 * x64.abs() * (1 + erf.abs()), 8, "unary gelu, every bf16 in the normal range")


# ---- fluxmi_resize_bilinear --------------------------------------------------------------------------------------------------------------------
def resize_inputs(B, Hi, Wi, C, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, Hi, Wi, C, generator=g) * (1 + torch.rand(C, generator=g))).bfloat16()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", CHANNELS)
def test_resize_bilinear_against_fp64(ops, dev, C, B):
    worst = 0.0
    for (Hi, Wi), (Ho, Wo) in SIZES:
        x = resize_inputs(B, Hi, Wi, C, hr.seed_of("resize", Hi, Wi, Ho, Wo, C, B))
        x64 = x.double().permute(0, 3, 1, 2)
        ref = dr.resize_ac(x64, Ho, Wo, True).permute(0, 2, 3, 1)
        A = dr.resize_taps_abs(x64, Ho, Wo).permute(0, 2, 3, 1)
        what = f"resize {Hi}x{Wi}->{Ho}x{Wo} C={C} B={B}"
        dense = ops.resize_bilinear(x.to(dev), (Ho, Wo))
        assert tuple(dense.shape) == (B, Ho, Wo, C)
        worst = max(worst, gate(dense, ref, A, 8, what))
        if (Hi, Wi) == (Ho, Wo):
            assert torch.equal(bits(dense.cpu()), bits(x)), f"{what}: the identity resize must be exact"
        # a channel window of a wider pixel buffer whose other channels are NaN, into a window of a sentinel-filled output
        ibuf, iwin = window(dev, x.shape, 8, 16, x)
        obuf, owin = window(dev, (B, Ho, Wo, C), 16, 8)
        assert ops.resize_bilinear(iwin, (Ho, Wo), out=owin).data_ptr() == owin.data_ptr()
        assert torch.equal(bits(owin.cpu()), bits(dense.cpu())), f"{what}: a strided run differs from the dense one"
        assert frame_intact(obuf, 16, C) and frame_intact(ibuf, 8, C), what
        # the fused add: bf16(bf16(resize) + add)
        g = torch.Generator().manual_seed(hr.seed_of("resize add", Hi, Wi, Ho, Wo, C, B))
        add = torch.randn(B, Ho, Wo, C, generator=g).bfloat16()
        abuf, awin = window(dev, add.shape, 8, 8, add)
        fused = ops.resize_bilinear(x.to(dev), (Ho, Wo), add=awin)
        gate(fused, ref + add.double(), A, 8, what + " + add", extra=U * ref.abs())
        assert torch.equal(bits(fused.cpu()), bits((dense.cpu().float() + add.float()).bfloat16())), f"{what}: the fused add is not bf16(bf16(resize) + add)"
        assert torch.equal(bits(ops.resize_bilinear(x.to(dev), (Ho, Wo))), bits(dense)), f"{what}: two runs differ"
        alone = ops.resize_bilinear(x[B - 1:].to(dev), (Ho, Wo))
        assert torch.equal(bits(alone[0]), bits(dense[B - 1])), f"{what}: a sample alone differs from the same sample in a batch"
    print(f"resize_bilinear C={C} B={B}: worst err / bound {worst:.3f}")


def test_resize_bilinear_equals_torch_on_fp32_coordinates(ops, dev):
    """torch's own align_corners=True resize of the same bf16 tensor, computed in fp32 on the host: the source pixels and weights agree, so
    the two differ by fp32 blend order alone -- at most one bf16 ulp, on a small share.  A weight that is off by an ulp of the source
    coordinate fails this (a blend at l = 1/2 of two bf16 values is an exact tie: with the coordinate contracted into an fma 1.4 % of the
    outputs round the other way), which the fp64 gate above, one bf16 rounding wide, cannot see."""
    x = resize_inputs(2, 19, 23, 64, 5)
    want = F.interpolate(x.float().permute(0, 3, 1, 2), size=(37, 41), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).bfloat16()
    got = ops.resize_bilinear(x.to(dev), (37, 41)).cpu()
    A = dr.resize_taps_abs(x.double().permute(0, 3, 1, 2), 37, 41).permute(0, 2, 3, 1)
    err = (got.double() - want.double()).abs()
    tol = 2.0 ** -7 * want.double().abs() + 8 * 2.0 ** -24 * A
    share = float((bits(got) == bits(want)).float().mean())
    print(f"resize vs torch fp32 on the host: worst err / tol {float((err / tol.clamp_min(1e-300)).max()):.3f}, {int((err > tol).sum())} beyond, "
          f"bit-equal share {share:.5f}")
    assert bool((err <= tol).all()), "more than one bf16 ulp (or the fp32 chain's error) apart"
    assert share >= 0.99


def test_resize_refusals(ops, dev):
    x = torch.zeros(1, 4, 4, 12, dtype=torch.bfloat16, device=dev)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.resize_bilinear(x, (3, 3))
    with pytest.raises(ValueError, match=">= 1 x 1"):
        ops.resize_bilinear(x[..., :8], (0, 3))
    with pytest.raises(ValueError, match="ONE pixel stride"):
        ops.resize_bilinear(torch.zeros(1, 4, 8, 8, dtype=torch.bfloat16, device=dev)[:, ::2], (3, 3))
    with pytest.raises(ValueError, match="kind="):
        ops.unary(x, "tanh")
    with pytest.raises(ValueError, match="normalize="):
        ops.depth_to_map(torch.zeros(1, 4, 4, device=dev), (4, 4), "max")


# ---- patch rows, the stride-2 convolution, the head's last convolution --------------------------------------------------------------------------
def test_patchify_rect_equals_the_definition(ops, dev):
    for B, gh, gw in ((1, 1, 1), (2, 3, 5), (3, 2, 7), (1, 4, 4)):
        pix = torch.randn(B, 3, 14 * gh + 3, 14 * gw + 5, generator=torch.Generator().manual_seed(gh * 10 + gw)).bfloat16()
        got = ops.patchify_rect(pix.to(dev), 14, gh, gw, 640).cpu()
        want = F.unfold(pix[:, :, :14 * gh, :14 * gw].float(), kernel_size=14, stride=14).transpose(1, 2).reshape(B * gh * gw, 588).bfloat16()
        assert torch.equal(bits(got[:, :588]), bits(want)) and not got[:, 588:].any(), (B, gh, gw)
        if gh == gw:
            assert torch.equal(bits(got), bits(ops.patchify(pix.to(dev), 14, gh, 640).cpu()))


# an unread border and a padded K;  K exactly C P P;  one patch per image and a pad of a single 8-vector
SQUARE_PATCH_CASES = [(2, 3, 31, 30, 14, 2, 640), (1, 2, 4, 4, 2, 2, 8), (3, 3, 14, 14, 14, 1, 592)]


@pytest.mark.parametrize("case", SQUARE_PATCH_CASES, ids=vr.case_id)
def test_patchify_square_equals_rect_and_the_definition(ops, dev, case):
    """fluxmi_patchify is fluxmi_patchify_rect's gather at grid_h = grid_w"""
    B, C, H, W, P, G, Kp = case
    pix = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(hr.seed_of("patchify", case))).bfloat16()
    kc = C * P * P
    want = F.unfold(pix[:, :, :G * P, :G * P].float(), kernel_size=P, stride=P).transpose(1, 2).reshape(B * G * G, kc).bfloat16()
    sq, rect = ops.patchify(pix.to(dev), P, G, Kp).cpu(), ops.patchify_rect(pix.to(dev), P, G, G, Kp).cpu()
    assert tuple(sq.shape) == tuple(rect.shape) == (B * G * G, Kp)
    assert torch.equal(bits(sq), bits(rect))
    assert torch.equal(bits(sq[:, :kc]), bits(want)) and not bits(sq[:, kc:]).any()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (5, 7)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_stride2_gather_equals_the_definition(ops, dev, hw, B):
    """conv3x3_s2's patch matrix at the narrowest channel count (one 8-vector per tap), odd and even sizes"""
    Hi, Wi = hw
    x = torch.randn(B, Hi, Wi, 8, generator=torch.Generator().manual_seed(hr.seed_of("s2 gather", hw, B))).bfloat16()
    Ho, Wo = ops.conv3x3_s2_hw(Hi, Wi)
    col = ops.im2col3x3_s2(x.to(dev)).cpu()
    assert tuple(col.shape) == (B * Ho * Wo, 72)
    assert torch.equal(bits(col), bits(s2_patch64(x).bfloat16()))


S2_CASES = [(2, 1, 1, 64, 128), (2, 3, 5, 64, 128), (1, 4, 4, 128, 256), (1, 37, 37, 128, 128)]


def s2_patch64(x):
    """x bf16 [B, Hi, Wi, C] -> fp64 [B Ho Wo, 9 C], columns (dy, dx, c), of Conv2d(3, stride 2, padding 1)"""
    B, Hi, Wi, C = x.shape
    u = F.unfold(x.double().permute(0, 3, 1, 2), kernel_size=3, stride=2, padding=1)  # [B, C * 9, L], rows (c, dy, dx)
    L = u.shape[-1]
    return u.view(B, C, 9, L).permute(0, 3, 2, 1).reshape(B * L, 9 * C)


@pytest.mark.parametrize("case", S2_CASES, ids=vr.case_id)
def test_conv3x3_stride2_against_fp64(ops, dev, case):
    B, Hi, Wi, C, Cout = case
    Ho, Wo = ops.conv3x3_s2_hw(Hi, Wi)
    gots, refs, mags = [], [], []
    for rep in range(vr.conv_reps(B * Ho * Wo, Cout)):
        g = torch.Generator().manual_seed(hr.seed_of("s2", case, rep))
        x = torch.randn(B, Hi, Wi, C, generator=g).bfloat16()
        w = (torch.randn(Cout, C, 3, 3, generator=g) * (9 * C) ** -0.5).bfloat16()
        bias = torch.randn(Cout, generator=g).bfloat16()
        w2 = w.permute(0, 2, 3, 1).reshape(Cout, 9 * C).contiguous()
        patch = s2_patch64(x)
        # the patch matrix is that of Conv2d(stride=2, padding=1), and the kernel's gather equals it bit for bit
        conv = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), bias.double(), stride=2, padding=1).permute(0, 2, 3, 1).reshape(-1, Cout)
        assert tuple(conv.shape) == (B * Ho * Wo, Cout) and (patch @ w2.double().T + bias.double() - conv).abs().max() < 1e-12
        col = ops.im2col3x3_s2(x.to(dev)).cpu()
        assert torch.equal(col.double(), patch), f"im2col3x3_s2 {case}: the gather differs from the definition"
        got = ops.conv3x3_s2(x.to(dev), w2.to(dev), bias.to(dev))
        assert tuple(got.shape) == (B, Ho, Wo, Cout)
        gots.append(got.cpu().reshape(-1, Cout)), refs.append(vr.linear_ref(patch, w2, bias)), mags.append(vr.gemm_mag(patch, w2, bias)[0])
        assert torch.equal(bits(ops.conv3x3_s2(x.to(dev), w2.to(dev), bias.to(dev))), bits(got)), "two runs differ"
    ex, worst = vr.gate_gemm(torch.cat(gots), torch.cat(refs), torch.cat(mags), 1.0, 0.99, f"conv3x3 stride 2 {case}")
    print(f"conv3x3 stride 2 {case}: bit-exact share {ex:.4f}, worst err / tol {worst:.3f}")


@pytest.mark.parametrize("C", [8, 32, 96])
def test_depth_head_against_fp64(ops, dev, C):
    g = torch.Generator().manual_seed(C)
    x = torch.relu(torch.randn(3, 9, 11, C, generator=g)).bfloat16()
    w = (torch.randn(C, generator=g) / C).bfloat16()
    bias = torch.tensor([0.05]).bfloat16()
    ref = torch.relu((x.double() * w.double()).sum(-1) + bias.double())
    A = (x.double() * w.double()).abs().sum(-1) + bias.double().abs()
    ibuf, iwin = window(dev, x.shape, 8, 8, x)
    got = ops.depth_head(iwin, w.to(dev), bias.to(dev))
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 9, 11)
    err = (got.cpu().double() - ref).abs()
    assert bool((err <= MARGIN * (C + 1) * 2.0 ** -24 * A).all()), float((err / A.clamp_min(1e-300)).max())
    assert bool((ref == 0).any()) and bool((got.cpu()[ref == 0] == 0).all()), "the ReLU"
    assert torch.equal(ops.depth_head(x[1:2].to(dev), w.to(dev), bias.to(dev))[0], got[1])


# ---- fluxmi_depth_to_map ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", ["minmax", "raw"])
@pytest.mark.parametrize("case", dr.MAP_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}to{c[1][0]}x{c[1][1]}")
def test_depth_to_map_equals_the_reference(ops, dev, case, normalize):
    (h, w), (H, W) = case
    d = dr.depth_samples(3, h, w, 1)
    if normalize == "raw":
        d[0] *= 40.0  # beyond 255: the clamp
    t = dr.depth_to_map_f64(d, H, W, normalize)
    want, excused = dr.map_bytes(t), dr.map_excused(t)
    assert excused.mean() <= 0.01
    # the depth as a window of a wider fp32 buffer, the map as a window of a sentinel-filled byte buffer (once dword-aligned, once not)
    dbuf = torch.full((3, h + 1, w + 5), float("nan"), device=dev)
    dbuf[:, :h, 2:2 + w] = torch.from_numpy(d).to(dev)
    for off in (4, 3):
        obuf = sentinel_like((3, H + 2, (3 * W + 12) // 2 + 1), dev).view(torch.uint8)
        owin = obuf[:, 1:H + 1, off:off + 3 * W].unflatten(-1, (W, 3))
        got = ops.depth_to_map(dbuf[:, :h, 2:2 + w], (H, W), normalize, out=owin)
        assert got.data_ptr() == owin.data_ptr()
        o = owin.cpu().numpy()
        assert np.array_equal(o[..., 0], o[..., 1]) and np.array_equal(o[..., 0], o[..., 2]), "the three channels differ"
        bad = o[..., 0] != want
        assert not (bad & ~excused).any(), (case, normalize, off, int((bad & ~excused).sum()), np.argwhere(bad & ~excused)[:4])
        assert (np.abs(o[..., 0].astype(int) - want.astype(int)) <= 1).all()
        full = obuf.cpu().clone()
        full[:, 1:H + 1, off:off + 3 * W] = sentinel_like((3, H + 2, (3 * W + 12) // 2 + 1)).view(torch.uint8)[:, 1:H + 1, off:off + 3 * W]
        assert torch.equal(full, sentinel_like((3, H + 2, (3 * W + 12) // 2 + 1)).view(torch.uint8)), "the frame around the map was written"
    dense = ops.depth_to_map(torch.from_numpy(d).to(dev), (H, W), normalize)
    assert np.array_equal(dense.cpu().numpy(), o), "a strided run differs from the dense one"
    assert torch.equal(ops.depth_to_map(torch.from_numpy(d).to(dev), (H, W), normalize), dense), "two runs differ"
    assert torch.equal(ops.depth_to_map(torch.from_numpy(d[1:2]).to(dev), (H, W), normalize)[0], dense[1]), "a sample alone differs"
    print(f"depth_to_map {case} {normalize}: excused share {excused.mean():.4f} (cap 0.01), mismatches among them {int((bad & excused).sum())}")


def test_depth_to_map_constant_image_and_end_points(ops, dev):
    const = torch.full((2, 7, 9), 3.25, device=dev)
    assert not ops.depth_to_map(const, (20, 30)).any(), "a constant image gives 0"
    d = torch.from_numpy(dr.depth_samples(2, 12, 15, 2)).to(dev)
    m = ops.depth_to_map(d, (12, 15)).cpu().numpy()[..., 0]
    for b in range(2):
        assert m[b].min() == 0 and m[b].max() == 255
    big = torch.from_numpy(dr.depth_samples(1, 300, 300, 3)).to(dev)  # 22 reduction chunks, the last one ragged
    big[0, 299, 299], big[0, 150, 7] = 1000.0, -50.0
    m = ops.depth_to_map(big, (300, 300)).cpu().numpy()[0, ..., 0]
    assert m[299, 299] == 255 and m[150, 7] == 0 and 0 < m[0, 0] < 255


# ---- the attention kernel at the longest sequence the estimator admits ------------------------------------------------------------------------
def test_vision_attention_at_the_longest_sequence(ops, dev):
    """74 x 74 + 1 = 5477 tokens in 5632 rows (depth_resolution 1036, square): past the 1024 the helper-kernel tests reach"""
    from modules.depth import MAX_TOKENS

    L, H, D = MAX_TOKENS, 2, 64
    Lp = (L + 255) // 256 * 256
    q, k, v, _, vb, scale, _ = hr.attention_inputs(L, H, D, "vision", hr.seed_of("depth attn", L))
    pad = lambda t: F.pad(t, (0, 0, 0, Lp - t.shape[1]))  # noqa: E731
    q, k, v = pad(q), pad(k), pad(v)
    out = ops.vision_attention(q.to(dev), k.to(dev), v.transpose(1, 2).contiguous().to(dev), L, H, D, scale, v_bias=vb.to(dev))
    ok, worst = hr.attention_gate(out[0, :L].cpu(), hr.attention_ref(q[0], k[0], v[0], L, H, D, scale, False, None, vb))
    print(f"vision_attention L={L} Lp={Lp}: worst err / tol {worst:.3f}")
    assert ok, worst


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(dev):
    """(config, state dict, the native model on the GPU, per grid: pixel values B = 3 and the fp64 / bf16-rounded reference features and depth)"""
    from fluxmi import synth
    from modules.depth import DepthAnythingNative

    cfg = dr.tiny_config()
    sd = synth.make_depth_anything_state_dict(cfg, 0)
    nat = DepthAnythingNative(cfg)
    nat.load_state_dict(sd, strict=True)
    nat = nat.to(device=dev, dtype=torch.bfloat16)
    sd64 = {k: v.double() for k, v in sd.items()}
    refs = {}
    with torch.no_grad():
        for g in dr.GRIDS:
            pix = dr.pixel_values(3, *g)
            f64, fbf = dr.backbone(sd64, cfg, pix), dr.backbone(sd, cfg, pix, torch.bfloat16)
            refs[g] = dict(pix=pix, f64=f64, fbf=fbf, d64=dr.decoder(sd64, cfg, f64, *g), dbf=dr.decoder(sd, cfg, fbf, *g, torch.bfloat16))
    return cfg, sd, nat, refs


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("grid", dr.GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_backbone_and_depth_against_the_fp64_reference(dev, tiny, grid, B):
    cfg, sd, nat, refs = tiny
    r = refs[grid]
    gh, gw = grid
    pix = r["pix"][:B].to(dev)
    feats = nat.features(pix)
    assert len(feats) == 4 and all(tuple(f.shape) == (B, gh, gw, 128) and f.dtype == torch.bfloat16 for f in feats)
    for i, f in enumerate(feats):
        got = f.reshape(B, gh * gw, 128)
        assert torch.isfinite(got).all()
        e, yard = dr.rel_l2(got, r["f64"][i][:B]), dr.rel_l2(r["fbf"][i][:B], r["f64"][i][:B])
        print(f"DEPTH_PARITY grid {gh}x{gw} B={B} tap {i + 1}: native {e:.3e}, bf16-rounded reference {yard:.3e}, ratio {e / yard:.3f} (gate 1.5)")
        assert e <= 1.5 * yard, (i, e, yard)
    depth = nat(pix)
    assert depth.dtype == torch.float32 and tuple(depth.shape) == (B, 14 * gh, 14 * gw) and torch.isfinite(depth).all()
    e, yard = dr.rel_l2(depth, r["d64"][:B]), dr.rel_l2(r["dbf"][:B], r["d64"][:B])
    print(f"DEPTH_PARITY grid {gh}x{gw} B={B} depth: native {e:.3e}, bf16-rounded reference {yard:.3e}, ratio {e / yard:.3f} (gate 1.5)")
    assert e <= 1.5 * yard, (e, yard)
    # the decoder alone, on the reference's own bf16 features: its own share of the error
    dec = nat.decode([f[:B].reshape(B, gh, gw, 128).bfloat16().to(dev) for f in r["fbf"]])
    assert dr.rel_l2(dec, r["d64"][:B]) <= 1.5 * yard
    assert torch.equal(nat(pix), depth), "two runs differ"


def test_large_geometry_shapes_need_no_padding(dev):
    """Depth Anything Large: 256 / 512 / 1024 / 1024, fusion 256, head 128 -> 32 are the kernels' shapes as they stand"""
    from fluxmi import synth
    from modules.depth import DepthAnythingNative

    cfg = synth.depth_anything_config("large", num_hidden_layers=2, out_indices=[1, 1, 2, 2])
    nat = DepthAnythingNative(cfg)
    assert nat.padded_sizes() == dict(neck=[256, 512, 1024, 1024], fusion=256, head1=128, head=32) and nat.head_dim == 64


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("control", [True, False], ids=["depth_model", "controlnet"])
def test_pipeline_depth_anything(dev, tiny, control):
    from PIL import Image

    import preprocess_ref as pr
    from modules.depth import depth_input_size
    from test_preprocess_gpu import tiny_pipeline

    cfg, sd, nat, _ = tiny
    pipe = tiny_pipeline(dev, control)
    g = torch.Generator().manual_seed(1)
    prompt = {"txt": 0.1 * torch.randn(1, 32, 128, generator=g), "vec": torch.randn(1, 64, generator=g)}
    photo = pr.family("smooth", 90, 60, seed=9)
    name = "control_image" if control else "controlnet_image"
    kw = dict(width=64, height=96, num_steps=4, seed=7, silent=True, output_type="latent", **({} if control else dict(control_mode=1)))

    def gen(**k):
        torch.manual_seed(5)  # the VAE encoder's Gaussian sample
        return pipe.generate(prompt, **kw, **k)

    edges = pipe.preprocess_control(photo, "canny", 64, 96)
    before = gen(**{name: edges}), gen(**{name: photo}, control_preprocess="canny")
    with pytest.raises(ValueError, match="depth_path"):
        gen(**{name: photo}, control_preprocess="depth_anything")
    pipe.depth_model = nat
    # requests without the kind: what they computed without a depth model, bit for bit
    assert torch.equal(gen(**{name: edges}), before[0]) and torch.equal(gen(**{name: photo}, control_preprocess="canny"), before[1])
    assert torch.equal(gen(**{name: edges}, control_preprocess=None), before[0])

    dmap = pipe.preprocess_control(photo, "depth_anything", 64, 96, depth_resolution=56)
    assert dmap.dtype == torch.uint8 and dmap.device.type == "cpu" and tuple(dmap.shape) == (96, 64, 3)
    assert int(dmap.max()) - int(dmap.min()) >= 128 and torch.equal(dmap[..., 0], dmap[..., 2])
    # the steps, restated: resize to the request, DPTImageProcessor's input, the model, the map of ITS depth by the reference
    resized = Image.fromarray(photo).resize((64, 96), Image.LANCZOS)
    assert depth_input_size(64, 96, 56) == (56, 84)
    depth = nat(nat.preprocess(resized, 56).to(dev))
    assert tuple(depth.shape) == (1, 84, 56)
    t = dr.depth_to_map_f64(depth.cpu().numpy(), 96, 64)
    bad = dmap.numpy()[..., 0] != dr.map_bytes(t)[0]
    assert not (bad & ~dr.map_excused(t)[0]).any()
    raw = pipe.preprocess_control(photo, "depth_anything", 64, 96, depth_resolution=56, depth_normalize="raw")
    assert raw.max() <= 3 and not torch.equal(raw, dmap), "the synthetic depth is below 3: raw writes it unscaled"

    from_map = gen(**{name: dmap})
    assert torch.isfinite(from_map).all() and not torch.equal(from_map, before[0])
    got = gen(**{name: photo}, control_preprocess="depth_anything", depth_resolution=56)
    assert torch.equal(got, from_map), "photo + control_preprocess differs from the map itself"
    other = gen(**{name: photo}, control_preprocess="depth_anything", depth_resolution=70, depth_normalize="raw")
    assert torch.equal(other, gen(**{name: pipe.preprocess_control(photo, "depth_anything", 64, 96, depth_resolution=70, depth_normalize="raw")}))
    assert not torch.equal(other, from_map)
