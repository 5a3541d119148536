"""fp64 references of the autoencoder's convolutions (the implicit GEMM of csrc/gemm.hip `CONV`, fluxmi_im2col3x3 of csrc/vae.hip, the 1x1 /
attention GEMMs), their seeded inputs, case tables and gates, and a call recorder that checks every launch of a whole decode / encode on
the very input it received.  Shared by tests/test_vae_kernels_gpu.py (kernel vs reference) and tests/test_vae_refs_cpu.py (which proves
that each gate rejects a wrong kernel and is attainable in fp32).

Every reference works in fp64 on the bf16 input VALUES and rounds only where the kernels document a rounding:
  patch matrix   a gather, exact: source = (o * stride + d - pad) / rep, zero outside (csrc/vae.hip, the comment of im2col3x3_kernel)
  conv / linear  h = bf16(a . w^T + bias); with a residual bf16(resid + bf16(gate * h)) (csrc/gemm_epilogue.h, EPI_GATE_RESID)
groupnorm, softmax and the streaming attention are helper_refs' and vae_attention_ref's, unchanged.

`mut=` selects a deliberately WRONG variant, each modelling one plausible slip of the kernel (MUTANTS); mut=None is the reference.
"""
import torch

import helper_refs as hr
import vae_attention_ref as var
from helper_refs import rbf64, seed_of
from parity_util import accum_noise, assert_close_mag, round_fp64_to_bf16

TILE_M = 128  # rows of one tile of the implicit kernel (launch_tile<128, 128, ...> in csrc/gemm.hip)
GRID1D_THREADS = 65535 * 16 * 256  # the most threads one im2col launch gets (grid1d in csrc/vae.hip); vectors past it take a second loop trip

MUTANTS = {
    "sym_pad_stride2": "mode -2 padded on all four sides",
    "up_src_plus1": "mode 2 source row (yy + 1) >> 1",
    "base_of_first_row": "every row of a 128-row tile uses the image index of the tile's first row",
    "wrap_x": "an x tap outside the image reads the neighbouring row's pixel instead of zero",
    "taps_transposed": "dy and dx exchanged",
    "cblock_reversed": "the 64-channel blocks of a tap in reverse order (C >= 128)",
    "gate_ones": "the gate ignored",
    "resid_prev_pixel": "the residual of the previous pixel",
    "drop_last_tile_row": "the last row of a ragged last tile left unwritten",
}
PATCH_MUTANTS = ("sym_pad_stride2", "up_src_plus1", "base_of_first_row", "wrap_x", "taps_transposed", "cblock_reversed")


# ---- geometry ------------------------------------------------------------------------------------------------------------------
def mode_params(mode):
    """(stride, pad, rep) of csrc/vae.hip:20-25"""
    return {1: (1, 1, 1), 2: (1, 1, 2), -2: (2, 0, 1)}[mode]


def out_hw(Hi, Wi, mode):
    return (Hi // 2, Wi // 2) if mode == -2 else (Hi * mode, Wi * mode)


def _fdiv(a, b):
    return torch.div(a, b, rounding_mode="floor")


def patch_rows(x, mode, rows=None, mut=None):
    """Rows `rows` (default: all) of the patch matrix of x [B, Hi, Wi, C], in x's dtype and on x's device: [len(rows), 9 C], columns in
    (dy, dx, c) order.  Plain index arithmetic from the definition: tap (dy, dx) of output pixel (b, yo, xo) is the input pixel
    ((yo * stride + dy - pad) / rep, (xo * stride + dx - pad) / rep) of image b, zero when the coordinate before the division lies outside
    [0, Hi * rep) x [0, Wi * rep)."""
    B, Hi, Wi, C = x.shape
    stride, pad, rep = mode_params(mode)
    H, W = out_hw(Hi, Wi, mode)
    dev = x.device
    r = torch.arange(B * H * W, device=dev) if rows is None else rows.to(dev)
    b, rem = _fdiv(r, H * W), r % (H * W)
    if mut == "base_of_first_row":
        b = _fdiv(_fdiv(r, TILE_M) * TILE_M, H * W)
    yo, xo = _fdiv(rem, W), rem % W
    d = torch.arange(3, device=dev)
    lo = 1 if (mut == "sym_pad_stride2" and mode == -2) else pad
    yy, xx = yo[:, None] * stride + d - lo, xo[:, None] * stride + d - lo  # [M, 3] each, in the upsampled / padded frame
    ok_y, ok_x = (yy >= 0) & (yy < Hi * rep), (xx >= 0) & (xx < Wi * rep)
    sy, sx = _fdiv(yy, rep), _fdiv(xx, rep)
    if mut == "up_src_plus1" and mode == 2:
        sy = _fdiv(yy + 1, 2).clamp(max=Hi - 1)
    flat = (b[:, None, None] * Hi + sy[:, :, None]) * Wi + sx[:, None, :]  # [M, dy, dx]
    ok = ok_y[:, :, None] & ok_x[:, None, :]
    if mut == "wrap_x":  # only y is checked; x = -1 / Wi run into the neighbouring row (nothing before the first / after the last pixel)
        ok = ok_y[:, :, None] & (flat >= 0) & (flat < B * Hi * Wi)
    if mut == "taps_transposed":
        flat, ok = flat.transpose(1, 2), ok.transpose(1, 2)
    flat, ok = flat.reshape(-1, 9), ok.reshape(-1, 9)
    g = x.reshape(B * Hi * Wi, C)[flat.clamp(0, B * Hi * Wi - 1)]  # [M, 9, C]
    g = torch.where(ok[:, :, None], g, torch.zeros((), dtype=x.dtype, device=dev))
    if mut == "cblock_reversed" and C >= 128:
        g = g.reshape(-1, 9, C // 64, 64).flip(2)
    return g.reshape(-1, 9 * C)


def patch_matrix64(x, mode, mut=None):
    """x [B, Hi, Wi, C] bf16 -> fp64 [B*H*W, 9C], columns in (dy, dx, c) order"""
    return patch_rows(x, mode, mut=mut).double()


# ---- references ----------------------------------------------------------------------------------------------------------------
def linear_ref(a, w, bias, gate=None, resid=None, mut=None, rounded=True):
    """a [M, K], w [N, K] -> h = bf16(a . w^T + bias); with a residual [M, N]: bf16(resid + bf16(gate * h)).  Returns bf16 (rounded=False:
    the unrounded fp64 a . w^T + bias).  The rounding points are the ones test_gemm_split_k states for EPI_GATE_RESID."""
    acc = a.double() @ w.double().T
    if bias is not None:
        acc = acc + bias.double()
    if not rounded:
        return acc
    h = rbf64(acc)
    if resid is None:
        out = round_fp64_to_bf16(acc)
    else:
        g = torch.ones(w.shape[0], dtype=torch.float64) if mut == "gate_ones" else gate.double()
        r = resid.reshape(-1, w.shape[0]).double()
        if mut == "resid_prev_pixel":
            r = torch.roll(r, 1, 0)
        out = round_fp64_to_bf16(r + rbf64(g * h))
    if mut == "drop_last_tile_row" and out.shape[0] % TILE_M:
        out[-1] = hr.sentinel_like((out.shape[1],))
    return out


def conv3x3_ref(x, w2, bias, mode, gate=None, resid=None, mut=None, rounded=True):
    """x [B, Hi, Wi, C] bf16, w2 [Cout, 9C] with K ordered (dy, dx, c) -> [B*H*W, Cout] (see linear_ref)"""
    patch = patch_matrix64(x, mode, mut if mut in PATCH_MUTANTS else None)
    return linear_ref(patch, w2, bias, gate, resid, None if mut in PATCH_MUTANTS else mut, rounded)


# ---- gates (the project's: test_bf16_gemm's for the plain epilogue, test_gemm_split_k's for the residual one) -------------------------
def worst_ratio(got, ref, mag, ulps):
    g, r = got.detach().cpu().double(), ref.detach().cpu().double()
    m = mag.detach().cpu().double() if torch.is_tensor(mag) else torch.full_like(r, float(mag))
    tol = ulps * torch.maximum(r.abs(), m) * 2.0 ** -7
    err = (g - r).abs()
    return float((err / tol.clamp_min(1e-300)).max())  # tol = 0 (a zero row of a padded weight): 0 when exact, huge otherwise


def gemm_mag(a, w, bias, gate=None, resid=None):
    """(mag, ulps, min_exact) of the gate for out = linear_ref(a, w, bias, gate, resid)"""
    noise = accum_noise(a, w, 1.0)
    if resid is None:
        return noise, 1.0, 0.99
    h = rbf64(linear_ref(a, w, bias, rounded=False))
    gh = (gate.double() * h).abs()
    mag = torch.maximum(torch.maximum(noise * gate.double().abs()[None, :], gh), resid.reshape(-1, w.shape[0]).double().abs())
    return mag, 2.05, 0.95


def gate_gemm(got, ref, mag, ulps, min_exact, what):
    """Every output finite (assert_close_mag cannot see a NaN: an unwritten sentinel, or a tap that missed the zero page), every element
    within `ulps` bf16 ulps at max(|ref|, mag), bit-exact share >= min_exact.  Returns (bit-exact share, worst err / tol)."""
    got = got.detach().cpu().reshape(ref.shape)
    assert torch.isfinite(got.float()).all(), f"{what}: {int((~torch.isfinite(got.float())).sum())} outputs are not finite"
    ex = assert_close_mag(got, ref, mag=mag, ulps=ulps, min_exact=min_exact, what=what)
    return ex, worst_ratio(got, ref, mag, ulps)


# ---- inputs and cases ----------------------------------------------------------------------------------------------------------
# (B, Hi, Wi, C, Cout, mode); Hi x Wi is the INPUT grid.  The smallest shapes at which each piece of the gather's address arithmetic can go wrong:
CONV_CASES = [
    (3, 5, 7, 64, 128, 1),      # 35 pixels per image: one ragged tile holds three images
    (2, 9, 13, 128, 256, 1),    # 117 pixels per image: tile 0 ends 11 pixels into image 1; two N tiles
    (2, 5, 7, 192, 128, 2),     # mode 2, 140 pixels per image, cpk = 3 (the tap = kt / cpk divide)
    (2, 18, 26, 64, 384, -2),   # mode -2, 117 pixels per image, three N tiles
    (1, 1, 1, 64, 128, 1),      # only the centre tap is inside the image
    (1, 1, 1, 128, 128, 2),     # 1x1 -> 2x2
    (1, 2, 2, 64, 128, -2),     # 2x2 -> 1x1
    (1, 1, 200, 64, 128, 1),    # one row: every dy != 1 tap is outside
    (2, 200, 1, 64, 128, 1),    # one column: every dx != 1 tap is outside
    (1, 3, 130, 512, 128, 1),   # a tile that lies inside one image row; 72 K-steps
]
EPILOGUES = ("plain", "resid")
# the cases in which a 128-row tile holds rows of two images
STRADDLING_CASES = [c for c in CONV_CASES if c[0] > 1 and (out_hw(c[1], c[2], c[5])[0] * out_hw(c[1], c[2], c[5])[1]) % TILE_M]

# im2col: (B, Hi, Wi, C, mode) -- the same geometries at C = 8 (one vector per tap: conv_in's padded 3 channels), 16, 72 (9 vectors) and 128.
IM2COL_CASES = [(B, Hi, Wi, C, mode) for (B, Hi, Wi, _, _, mode) in CONV_CASES for C in (8, 16, 72, 128)]
# The last case is the only one whose vector count, 2 * 2732^2 * 9 * 2 = 268 697 664, exceeds GRID1D_THREADS = 268 431 360: the first
# 266 304 threads take a second trip of the grid-stride loop, and the last elements of `col` lie past index 2^31.  Checked on the GPU only,
# chunk by chunk (4.3 GB of patch matrix); the CPU module walks IM2COL_CASES[:-1].
IM2COL_BIG = (2, 1366, 1366, 16, 2)
IM2COL_CASES.append(IM2COL_BIG)


def im2col_vectors(B, Hi, Wi, C, mode):
    H, W = out_hw(Hi, Wi, mode)
    return B * H * W * 9 * (C // 8)


def conv_reps(M, Cout):
    """a bit-exact share says nothing about 128 values: cases with fewer than 400 outputs are repeated with fresh seeds and gated together"""
    return max(1, -(-400 // (M * Cout)))


def conv_inputs(case, rep=0):
    """(x [B, Hi, Wi, C], w2 [Cout, 9C], bias [Cout], gate [Cout] = 1 + 0.5 N(0, 1), resid [M, Cout]) bf16 on the host"""
    B, Hi, Wi, C, Cout, mode = case
    g = torch.Generator().manual_seed(seed_of("conv", case, rep))
    H, W = out_hw(Hi, Wi, mode)
    x = torch.randn(B, Hi, Wi, C, generator=g).bfloat16()
    w2 = (torch.randn(Cout, 9 * C, generator=g) * (9 * C) ** -0.5).bfloat16()
    bias = torch.randn(Cout, generator=g).bfloat16()
    gate = (1 + 0.5 * torch.randn(Cout, generator=g)).bfloat16()
    resid = torch.randn(B * H * W, Cout, generator=g).bfloat16()
    return x, w2, bias, gate, resid


def conv_case_ref(case, epi, rep=0, mut=None):
    """(inputs, ref bf16 [M, Cout], (mag, ulps, min_exact)) of one case and epilogue"""
    x, w2, bias, gate, resid = conv_inputs(case, rep)
    if epi == "plain":
        gate = resid = None
    ref = conv3x3_ref(x, w2, bias, case[5], gate, resid, mut=mut)
    return (x, w2, bias, gate, resid), ref, gemm_mag(patch_matrix64(x, case[5]), w2, bias, gate, resid)


def gate_conv_case(case, epi, run, what):
    """run(x, w2, bias, gate, resid, mode) -> [M, Cout] bf16, once per repetition; all repetitions gated together.  Returns (share, worst)."""
    B, Hi, Wi, C, Cout, mode = case
    H, W = out_hw(Hi, Wi, mode)
    gots, refs, mags = [], [], []
    for rep in range(conv_reps(B * H * W, Cout)):
        inp, ref, (mag, ulps, min_exact) = conv_case_ref(case, epi, rep)
        gots.append(run(*inp, mode).detach().cpu().reshape(ref.shape)), refs.append(ref), mags.append(mag)
    return gate_gemm(torch.cat(gots), torch.cat(refs), torch.cat(mags), ulps, min_exact, what)


def case_id(c):
    return "x".join(str(v) for v in c)


# ---- the stage walk ------------------------------------------------------------------------------------------------------------
WALK_PARAMS = dict(resolution=32, in_channels=3, ch=64, out_ch=3, ch_mult=[1, 2, 8], num_res_blocks=1, z_channels=16, scale_factor=0.3611,
                   shift_factor=0.1159)
WALK_B, WALK_LATENT = 2, (5, 6)  # 30 pixels at the mid block, 120 and 480 above: no resolution's pixel count per image is a multiple of 128

_COMMON_ARMS = {
    "im2col3x3 mode=1", "linear im2col K=576 resid", "groupnorm swish=1", "groupnorm swish=0",
    "conv3x3 implicit mode=1", "conv3x3 implicit mode=1 resid", "conv3x3 pad128 mode=1",
    "linear 1x1", "linear 1x1 resid", "linear V^T",
}
_GEMM_ATTN = {"linear Q K^T", "softmax_rows masked", "linear P V"}
_DECODE = _COMMON_ARMS | {"linear im2col K=144", "conv3x3 implicit mode=2"}  # conv_in from 16 channels; the two upsamples
_ENCODE = _COMMON_ARMS | {"linear im2col K=72", "conv3x3 implicit mode=-2", "conv3x3 pad128 mode=-2"}  # conv_in from 3 (padded to 8)
EXPECTED_ARMS = {
    ("decode", "gemm"): frozenset(_DECODE | _GEMM_ATTN), ("decode", "streaming"): frozenset(_DECODE | {"vae_attention"}),
    ("encode", "gemm"): frozenset(_ENCODE | _GEMM_ATTN), ("encode", "streaming"): frozenset(_ENCODE | {"vae_attention"}),
}


def walk_autoencoder(attention="gemm", device="cpu"):
    import vae_oracle as vo
    from modules.autoencoder import AutoEncoder, AutoEncoderParams

    ae = AutoEncoder(AutoEncoderParams(**WALK_PARAMS))
    ae.load_state_dict(vo.synth_state_dict({k: v.shape for k, v in ae.state_dict().items()}, seed=7), strict=True)
    ae.attention = attention
    return ae.to(device)


def walk_input(direction):
    """decode: z [2, 16, 5, 6]; encode: an image [2, 3, 20, 24] in [-1, 1] (5 x 6 at the mid block either way)"""
    g = torch.Generator().manual_seed(seed_of("walk", direction))
    h, w = WALK_LATENT
    if direction == "decode":
        return torch.randn(WALK_B, WALK_PARAMS["z_channels"], h, w, generator=g)
    n = 1 << (len(WALK_PARAMS["ch_mult"]) - 1)
    return (torch.rand(WALK_B, 3, h * n, w * n, generator=g) * 2 - 1).bfloat16().float()


def walk_stages(ae, direction, inp):
    """AutoEncoder.decode / encode_moments stage by stage (they refuse CPU tensors; their stage methods do not): the CPU module's driver"""
    if direction == "decode":
        d = ae.decoder
        h = (inp.float() / ae.scale_factor + ae.shift_factor).permute(0, 2, 3, 1).to(torch.bfloat16).contiguous()
        h = ae._conv3(h, d.conv_in)
        h = ae._resnet(h, d.mid.block_1)
        h = ae._attn(h, d.mid.attn_1)
        h = ae._resnet(h, d.mid.block_2)
        for i_level in reversed(range(d.num_resolutions)):
            for i_block in range(d.num_res_blocks + 1):
                h = ae._resnet(h, d.up[i_level].block[i_block])
            if i_level != 0:
                h = ae._conv3(h, d.up[i_level].upsample.conv, upsample=2)
        return ae._conv3(ae._norm(h, d.norm_out, True), d.conv_out)
    e = ae.encoder
    h = inp.permute(0, 2, 3, 1).to(torch.bfloat16).contiguous()
    h = ae._conv3(h, e.conv_in)
    for i_level in range(e.num_resolutions):
        for i_block in range(e.num_res_blocks):
            h = ae._resnet(h, e.down[i_level].block[i_block])
        if i_level != e.num_resolutions - 1:
            h = ae._conv3(h, e.down[i_level].downsample.conv, upsample=-2)
    h = ae._resnet(h, e.mid.block_1)
    h = ae._attn(h, e.mid.attn_1)
    h = ae._resnet(h, e.mid.block_2)
    return ae._conv3(ae._norm(h, e.norm_out, True), e.conv_out)


# ---- call recorder -------------------------------------------------------------------------------------------------------------
def _host(t):
    return None if t is None else t.detach().cpu().clone()


class Recorder:
    """The launches of one decode / encode: kind, arm, clones of the inputs and of the output as they were at the call"""

    def __init__(self):
        self.records = []
        self._conv3 = []         # stack of (conv module, mode, has residual) of the _conv3 calls in flight
        self._linear_outs = set()  # data pointers of the outputs of earlier linear / softmax calls (kept alive by _keep)
        self._softmax_outs = set()
        self._keep = []

    def arms(self):
        return {r["arm"] for r in self.records}

    def add(self, kind, arm, out, **inputs):
        self._keep.append(out)
        self.records.append(dict(kind=kind, arm=arm, out=_host(out), **{k: _host(v) if torch.is_tensor(v) else v for k, v in inputs.items()}))
        return out


def record_calls(monkeypatch):
    """Wrap fluxmi.ops.conv3x3 / im2col3x3 / linear / groupnorm / softmax_rows / vae_attention (AutoEncoder looks them up as ops.X at call
    time) as they stand -- patch them with emulations BEFORE this call to drive the recorder without a GPU -- and AutoEncoder._conv3, which
    only tells the recorder which convolution a launch belongs to.  Returns the Recorder."""
    from fluxmi import _lib, ops
    from modules.autoencoder import AutoEncoder

    rec = Recorder()
    real = {n: getattr(ops, n) for n in ("conv3x3", "im2col3x3", "linear", "groupnorm", "softmax_rows", "vae_attention")}
    real_conv3 = AutoEncoder._conv3

    def _conv3(self, x, conv, upsample=1, resid=None):
        rec._conv3.append((conv, upsample, resid is not None))
        try:
            return real_conv3(self, x, conv, upsample, resid)
        finally:
            rec._conv3.pop()

    def conv3x3(x, w2, bias=None, upsample=1, resid=None, gate=None):
        out = real["conv3x3"](x, w2, bias, upsample, resid=resid, gate=gate)
        arm = "implicit"
        if rec._conv3:
            conv, mode, _ = rec._conv3[-1]
            assert mode == upsample
            arm = "implicit" if conv.out_channels == w2.shape[0] else "pad128"
        return rec.add("conv3x3", f"conv3x3 {arm} mode={upsample}" + (" resid" if resid is not None else ""), out, x=x, w2=w2, bias=bias,
                       mode=upsample, gate=gate, resid=resid)

    def im2col3x3(x, upsample=1):
        return rec.add("im2col3x3", f"im2col3x3 mode={upsample}", real["im2col3x3"](x, upsample), x=x, mode=upsample)

    def linear(x, W, bias=None, *a, **k):
        assert not a and set(k) <= {"epilogue", "gate", "resid", "out"}, "the autoencoder passed linear() an argument the recorder does not model"
        out = real["linear"](x, W, bias, **k)
        has_resid = k.get("epilogue", _lib.EPI_BF16) == _lib.EPI_GATE_RESID
        assert has_resid == (k.get("resid") is not None)
        if rec._conv3:
            arm = f"linear im2col K={x.shape[1]}" + (" resid" if has_resid else "")
        elif has_resid:
            arm = "linear 1x1 resid"
        elif x.data_ptr() in rec._softmax_outs:
            arm = "linear P V"
        elif bias is None and x.data_ptr() in rec._linear_outs and W.data_ptr() in rec._linear_outs:
            arm = "linear Q K^T"
        elif bias is None:
            assert x.shape[0] == x.shape[1] == W.shape[1], "a bias-free GEMM that is neither Q K^T nor the operand-swapped V^T"
            arm = "linear V^T"
        else:
            arm = "linear 1x1"
        rec._linear_outs.add(out.data_ptr())
        return rec.add("linear", arm, out, a=x, w=W, bias=bias, gate=k.get("gate") if has_resid else None, resid=k.get("resid"))

    def groupnorm(x, gamma, beta, swish=True, eps=1e-6):
        return rec.add("groupnorm", f"groupnorm swish={int(bool(swish))}", real["groupnorm"](x, gamma, beta, swish=swish, eps=eps), x=x, gamma=gamma,
                       beta=beta, swish=bool(swish), eps=eps)

    def softmax_rows(S, scale):
        out = real["softmax_rows"](S, scale)
        rec._softmax_outs.add(out.data_ptr())
        masked = bool(torch.isinf(S).any())
        return rec.add("softmax_rows", "softmax_rows masked" if masked else "softmax_rows", out, S=S, scale=float(scale))

    def vae_attention(q, k, vt, P, v_bias=None, out=None):
        return rec.add("vae_attention", "vae_attention", real["vae_attention"](q, k, vt, P, v_bias=v_bias, out=out), q=q, k=k, vt=vt, P=int(P), v_bias=v_bias)

    for name, fn in (("conv3x3", conv3x3), ("im2col3x3", im2col3x3), ("linear", linear), ("groupnorm", groupnorm), ("softmax_rows", softmax_rows),
                     ("vae_attention", vae_attention)):
        monkeypatch.setattr(ops, name, fn)
    monkeypatch.setattr(AutoEncoder, "_conv3", _conv3)
    return rec


def check_call(r, what=""):
    """One record against its reference under that op's gate.  Returns (arm, worst err / tol or None, bit-exact share)."""
    what = f"{what}{r['arm']}"
    out = r["out"]
    if r["kind"] == "conv3x3":
        patch = patch_matrix64(r["x"], r["mode"])
        ref = linear_ref(patch, r["w2"], r["bias"], r["gate"], r["resid"])
        ex, worst = gate_gemm(out, ref, *gemm_mag(patch, r["w2"], r["bias"], r["gate"], r["resid"]), what)
        return r["arm"], worst, ex
    if r["kind"] == "linear":
        ref = linear_ref(r["a"], r["w"], r["bias"], r["gate"], r["resid"])
        ex, worst = gate_gemm(out, ref, *gemm_mag(r["a"], r["w"], r["bias"], r["gate"], r["resid"]), what)
        return r["arm"], worst, ex
    if r["kind"] == "im2col3x3":
        ref = patch_rows(r["x"], r["mode"])
        assert out.shape == ref.shape and torch.equal(hr.bits(out), hr.bits(ref)), f"{what}: the patch matrix differs from its definition"
        return r["arm"], 0.0, 1.0
    if r["kind"] == "groupnorm":
        ref = hr.groupnorm_ref(r["x"], r["gamma"], r["beta"], r["swish"], eps=r["eps"])
        ex = hr.gate_groupnorm(out, ref, what)
        return r["arm"], worst_ratio(out, ref, 0.25, 1.0), ex
    if r["kind"] == "softmax_rows":
        ref = hr.softmax_ref(r["S"], r["scale"])
        ex = hr.gate_softmax(out, ref, what)
        if r["arm"].endswith("masked"):
            assert bool((out[torch.isinf(r["S"])] == 0).all()), f"{what}: a masked column has a non-zero probability"
        return r["arm"], None, ex
    assert r["kind"] == "vae_attention"
    P = r["P"]
    q, k, v = r["q"][:, :P], r["k"][:, :P], r["vt"][:, :, :P].transpose(1, 2)
    f = var.assert_close(out[:, :P], var.gate(q, k, v, r["v_bias"]), what)
    return r["arm"], f["r_got"] / (var.MARGIN * max(1.0, f["r_model"])), None


def check_all(rec, what):
    """check_call on every record; prints one line per arm: launches, the worst err / tol and the lowest bit-exact share among them"""
    per_arm = {}
    for i, r in enumerate(rec.records):
        arm, worst, ex = check_call(r, f"{what} #{i} ")
        n, w, e = per_arm.get(arm, (0, None, None))
        per_arm[arm] = (n + 1, worst if w is None else (w if worst is None else max(w, worst)), ex if e is None else (e if ex is None else min(e, ex)))
    for arm in sorted(per_arm):
        n, w, e = per_arm[arm]
        print(f"{what} {arm}: {n} launches, worst err/tol {'-' if w is None else format(w, '.3f')}, lowest bit-exact share {'-' if e is None else format(e, '.5f')}")
    return per_arm


# ---- fp32 emulations of the six ops (torch on the host): what a correct fp32 kernel computes, for the CPU module ----------------------
def emul_linear(x, W, bias=None, *, epilogue=None, gate=None, resid=None, out=None):
    h = x.float() @ W.float().T
    if bias is not None:
        h = h + bias.float()
    h = h.bfloat16()
    if resid is not None:
        h = (resid.reshape(h.shape).float() + (gate.float() * h.float()).bfloat16().float()).bfloat16()
    if out is None:
        return h
    out.copy_(h)
    return out


def emul_conv3x3(x, w2, bias=None, upsample=1, resid=None, gate=None):
    B, Hi, Wi, _ = x.shape
    H, W = out_hw(Hi, Wi, upsample)
    if resid is not None and gate is None:
        gate = torch.ones(w2.shape[0], dtype=torch.bfloat16)
    return emul_linear(patch_rows(x.contiguous(), upsample), w2, bias, gate=gate, resid=resid).view(B, H, W, -1)


def emul_im2col3x3(x, upsample=1):
    """F.unfold on the upsampled / (0, 1, 0, 1)-padded image (test_im2col3x3's construction): independent of patch_rows"""
    import torch.nn.functional as F

    B, Hi, Wi, C = x.shape
    H, W = out_hw(Hi, Wi, upsample)
    xn = x.permute(0, 3, 1, 2).float()
    if upsample == 2:
        xn = F.interpolate(xn, scale_factor=2.0, mode="nearest")
    u = F.unfold(F.pad(xn, (0, 1, 0, 1)), kernel_size=3, stride=2) if upsample == -2 else F.unfold(xn, kernel_size=3, padding=1)
    return u.view(B, C, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 9 * C).bfloat16()


def emul_groupnorm(x, gamma, beta, swish=True, eps=1e-6):
    B, P, C = x.shape
    v = x.float().view(B, P, 32, C // 32)
    mean = v.mean((1, 3), keepdim=True)
    rstd = torch.rsqrt(((v - mean) ** 2).mean((1, 3), keepdim=True) + eps)
    y = ((v - mean) * rstd).view(B, P, C) * gamma.float() + beta.float()
    return (y * torch.sigmoid(y) if swish else y).bfloat16()


def emul_softmax_rows(S, scale):
    return torch.softmax(S.float() * scale, -1).bfloat16()


def emul_vae_attention(q, k, vt, P, v_bias=None, out=None):
    res = var.model(q[:, :P], k[:, :P], vt[:, :, :P].transpose(1, 2), v_bias)
    if out is None:
        return res
    out[:, :P] = res
    return out


EMULATIONS = dict(conv3x3=emul_conv3x3, im2col3x3=emul_im2col3x3, linear=emul_linear, groupnorm=emul_groupnorm, softmax_rows=emul_softmax_rows,
                  vae_attention=emul_vae_attention)
