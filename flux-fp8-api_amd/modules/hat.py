"""HAT -- the Hybrid Attention Transformer behind the HAT_SRx4 / HAT-L / Real_HAT_GAN_SRx4 and community "4x...HAT-L" upscalers -- on
fluxmi_window_attention16, fluxmi_channel_mean and fluxmi_channel_combine (csrc/window_attention16.hip).  This docstring is the definition
the code and tests/hat_ref.py follow; it is written from the public hat_arch.py as far as it is known:

  x     = (x - mean) * img_range, reflect-padded to multiples of the window (16);  mean = (0.4488, 0.4371, 0.4040), img_range = 1
  feat  = conv_first(x)                                                      3 -> C (embed_dim)
  body  : t = LayerNorm(feat) (patch_embed.norm);  RHAG^n;  LayerNorm (norm);  trunk = conv_after_body(t) + feat
  RHAG  : t + conv(OCAB(HAB^depth(t)))                                       layers.{i}: residual_group.blocks.{j}, .overlap_attn, conv ("1conv")
  HAB   : n = norm1(t);  t = t + proj(window_attention(qkv(n))) + 0.01 * CAB(n);  t = t + fc2(gelu(fc1(norm2(t))))
          window 16, shift 0 in even blocks and 8 in odd ones (the -100 mask of Swin), bias = table[relative_position_index_SA]; conv_scale
          is 0.01 in every published config and is not in the checkpoint
  CAB   : y = conv3x3(gelu(conv3x3(n)))  (C -> C / compress -> C);  y * sigmoid(W2 relu(W1 mean_HW(y) + b1) + b2)  (C -> C / squeeze -> C)
  OCAB  : n = norm1(t);  q, k, v = qkv(n);  each 16 x 16 query window attends to the 24 x 24 pixels around it -- nn.Unfold(24, stride 16,
          padding 4) of k and v, so positions outside the image are ZERO k / v that still take part in the softmax -- with
          bias = table[relative_position_index_OCA];  t = t + proj(attention);  t = t + fc2(gelu(fc1(norm2(t))))
  out   = conv_last(shuffle2(upsample.2(shuffle2(upsample.0(lrelu_0.01(conv_before_upsample(trunk)))))))  ("pixelshuffle"; x2 has no
          upsample.2) / img_range + mean, cropped to scale * (H, W)
  scale = head_dim^-1/2 on q in both attentions, the exact (erf) GELU, LayerNorm eps 1e-5.

On libfluxmi the network is laid out as modules/swinir.py lays out SwinIR: NHWC bf16 rows of Cp = C rounded up to 64 channels with pad
channels held at zero by zero weight rows / columns, LayerNorm on fluxmi_channel_norm, linears on the bf16 GEMM with its gate * y + x
epilogue for the residual sums, GELU on fluxmi_unary, heads zero-padded to 32 columns in qkv / proj, convolutions on fluxmi_conv3x3_dense in
windows of at most 64 outputs.  Both attentions are ONE launch of fluxmi_window_attention16 each (overlap 0 / 4); CAB's mean is
fluxmi_channel_mean and its squeeze MLP, gate and the HAB's three-way sum t + proj(..) + 0.01 * y * g are ONE fluxmi_channel_combine launch
(fp32 weights, one rounding).  PixelShuffle is a reshape / permute of the conv's output (data movement).  Every launch rounds to bf16 once.

Geometry (embed_dim, depths, heads, CAB and MLP widths, x2 / x4) is read from the checkpoint and every expected tensor is checked by name and
shape; keys may be wrapped in params_ema / params.  The relative_position_index_SA / _OCA buffers are taken from the file when present;
negative entries mean what they mean to torch's indexing (rows counted from the end) and are folded once, then every entry is checked against
the table's rows.  Without the buffers the indices are computed by the public formulas (index_sa / index_oca below): THAT BRANCH IS UNPINNED
-- written from memory of hat_arch.py, not compared with it.  attn_mask buffers are ignored (the mask is a function of the input size).
Refused by name: x3 and x8 upsamplers, windows other than 16, an overlap ratio other than 0.5, 3conv, ape, head_dim > 32, C > 256.  No HAT
code or checkpoint has been available here: key layout, parity with upstream and image quality are unverified (synthetic weights only).
"""
from __future__ import annotations

import re
from typing import Dict

import torch
import torch.nn.functional as F

from modules.swinir import LN_EPS, MEAN, _head_index, _pad1, _pad2, _up, unwrap
from modules.upscaler import UpscalerFormatError

WINDOW, OVERLAP, HEAD_PAD, CONV_SCALE = 16, 4, 32, 0.01
SA_ROWS, OCA_ROWS = (2 * WINDOW - 1) ** 2, (2 * WINDOW + 2 * OVERLAP - 1) ** 2  # 961, 1521
_BLOCK = re.compile(r"^layers\.(\d+)\.residual_group\.blocks\.(\d+)\.")
_IGNORED = re.compile(r"(relative_position_index(_SA|_OCA)?|attn_mask)$")


def is_hat(sd: dict) -> bool:
    """does the (possibly wrapped) state dict hold HAT's overlapping cross-attention or channel-attention blocks: read_upscaler's dispatch"""
    return any(".residual_group.overlap_attn." in k or ".conv_block.cab." in k for k in unwrap(sd))


def index_sa() -> torch.Tensor:
    """Swin's relative-position index at window 16: [256, 256], (ya - yb + 15) * 31 + (xa - xb + 15)"""
    co = torch.stack(torch.meshgrid(torch.arange(WINDOW), torch.arange(WINDOW), indexing="ij")).flatten(1)
    rel = (co[:, :, None] - co[:, None, :]).permute(1, 2, 0) + WINDOW - 1
    return rel[..., 0] * (2 * WINDOW - 1) + rel[..., 1]


def index_oca() -> torch.Tensor:
    """HAT's calculate_rpi_oca at window 16 / extended window 24: [256, 576].  The offsets key - query + (16 - 24 + 1) run from -22 to 16, and
    hat_arch.py indexes the table with them as they are; the loader folds the negative ones as torch's indexing does."""
    ext = WINDOW + 2 * OVERLAP
    ori = torch.stack(torch.meshgrid(torch.arange(WINDOW), torch.arange(WINDOW), indexing="ij")).flatten(1)
    big = torch.stack(torch.meshgrid(torch.arange(ext), torch.arange(ext), indexing="ij")).flatten(1)
    rel = (big[:, None, :] - ori[:, :, None]).permute(1, 2, 0) + WINDOW - ext + 1
    return rel[..., 0] * (WINDOW + ext - 1) + rel[..., 1]


def _index(sd, name: str, computed, rows: int, nk: int) -> torch.Tensor:
    idx = sd[name].long() if name in sd else computed()
    if tuple(idx.shape) != (WINDOW * WINDOW, nk):
        raise UpscalerFormatError(f"hat: {name} is {tuple(idx.shape)}, expected {(WINDOW * WINDOW, nk)} (window 16, overlap ratio 0.5)")
    idx = torch.where(idx < 0, idx + rows, idx)
    if int(idx.min()) < 0 or int(idx.max()) >= rows:
        raise UpscalerFormatError(f"hat: {name} holds entries in {int(idx.min())}..{int(idx.max())}, outside the bias table's {rows} rows")
    return idx.to(torch.int32).contiguous()


def infer_geometry(sd: Dict[str, torch.Tensor]) -> dict:
    """unwrapped HAT keys -> dict(embed_dim, depths, heads, mlp_hidden, ocab_hidden, compress, squeeze, num_feat, scale); every expected
    tensor is checked by name and shape, anything else is refused by name"""
    ks = list(sd)
    if "absolute_pos_embed" in sd:
        raise UpscalerFormatError("hat: this checkpoint uses ape (an absolute position embedding of a fixed image size); not supported")
    if "conv_first.weight" not in sd or not any(_BLOCK.match(k) for k in ks) or not is_hat(sd):
        raise UpscalerFormatError("hat: not a HAT checkpoint (no conv_first / layers.*.residual_group.blocks.* / overlap_attn / conv_block.cab)")
    C = int(sd["conv_first.weight"].shape[0])
    depths = {}
    for k in ks:
        m = _BLOCK.match(k)
        if m:
            i, j = int(m.group(1)), int(m.group(2))
            depths[i] = max(depths.get(i, 0), j + 1)
    n_layers = 1 + max(depths)
    if sorted(depths) != list(range(n_layers)):
        raise UpscalerFormatError(f"hat: layers {sorted(depths)} are not 0..{n_layers - 1}")
    depths = [depths[i] for i in range(n_layers)]
    if "layers.0.conv.weight" not in sd:
        raise UpscalerFormatError("hat: layers.0.conv is not a single 3x3 (a 3conv residual connection); only 1conv is supported")
    if "upsample.0.weight" not in sd or "conv_before_upsample.0.weight" not in sd:
        raise UpscalerFormatError("hat: the checkpoint has no conv_before_upsample.0 / upsample.0 (HAT reconstructs with pixelshuffle)")
    nf = int(sd["conv_before_upsample.0.weight"].shape[0])
    if "upsample.4.weight" in sd:
        raise UpscalerFormatError("hat: an x8 upsampler (upsample.0 / .2 / .4); only x2 and x4 are supported")
    if int(sd["upsample.0.weight"].shape[0]) == 9 * nf:
        raise UpscalerFormatError("hat: an x3 upsampler (upsample.0 has 9 * num_feat outputs); only x2 and x4 are supported")
    scale = 4 if "upsample.2.weight" in sd else 2
    if nf % 16 or not 16 <= nf <= 64:
        raise UpscalerFormatError(f"hat: num_feat={nf}: the reconstruction convolutions take a multiple of 16 in 16..64")
    heads = []
    for i in range(n_layers):
        g = f"layers.{i}.residual_group."
        for name, rows, what in ((g + "blocks.0.attn.relative_position_bias_table", SA_ROWS, "window"),
                                 (g + "overlap_attn.relative_position_bias_table", OCA_ROWS, "overlap")):
            t = sd.get(name)
            if t is None or t.ndim != 2:
                raise UpscalerFormatError(f"hat: the checkpoint has no {name}")
            if int(t.shape[0]) != rows:
                side = round(int(t.shape[0]) ** 0.5)
                why = (f"window {(side + 1) // 2}; only window {WINDOW} ({SA_ROWS} rows) is supported" if what == "window" else
                       f"an overlap ratio of {(side + 1 - 2 * WINDOW) / WINDOW:g} at window {WINDOW}; only an overlap ratio of 0.5 ({OCA_ROWS} rows) is supported")
                raise UpscalerFormatError(f"hat: {name} has {t.shape[0]} rows: {why}")
        heads.append(int(sd[g + "blocks.0.attn.relative_position_bias_table"].shape[1]))
        if C % heads[-1] or C // heads[-1] > HEAD_PAD:
            raise UpscalerFormatError(f"hat: layers.{i}: embed_dim {C} over {heads[-1]} heads: head_dim must divide and be <= {HEAD_PAD} (head_dim > 32 is not supported)")
    if _up(C, 64) > 256:
        raise UpscalerFormatError(f"hat: embed_dim {C} pads to {_up(C, 64)} channels, C > 256; fluxmi_conv3x3_dense reads at most 256")
    p0 = "layers.0.residual_group."
    dim = lambda name, d=0: int(sd[name].shape[d]) if name in sd else 0  # noqa: E731  a missing tensor is named by the shape check below
    hidden, hid2 = dim(p0 + "blocks.0.mlp.fc1.weight"), dim(p0 + "overlap_attn.mlp.fc1.weight")
    Cc, Cs = dim(p0 + "blocks.0.conv_block.cab.0.weight"), dim(p0 + "blocks.0.conv_block.cab.3.attention.1.weight")
    if not 1 <= Cs <= 64:
        raise UpscalerFormatError(f"hat: the channel attention squeezes to {Cs} channels; fluxmi_channel_combine takes 1..64")
    want = {"conv_first": (C, 3, 3, 3), "conv_after_body": (C, C, 3, 3), "conv_before_upsample.0": (nf, C, 3, 3), "upsample.0": (4 * nf, nf, 3, 3),
            "conv_last": (3, nf, 3, 3), "patch_embed.norm": (C,), "norm": (C,)}
    if scale == 4:
        want["upsample.2"] = (4 * nf, nf, 3, 3)
    for i in range(n_layers):
        g = f"layers.{i}.residual_group."
        want[f"layers.{i}.conv"] = (C, C, 3, 3)
        o = g + "overlap_attn."
        want.update({o + "norm1": (C,), o + "norm2": (C,), o + "qkv": (3 * C, C), o + "proj": (C, C), o + "mlp.fc1": (hid2, C), o + "mlp.fc2": (C, hid2)})
        tables = {o + "relative_position_bias_table": (OCA_ROWS, heads[i])}
        for j in range(depths[i]):
            p = f"{g}blocks.{j}."
            want.update({p + "norm1": (C,), p + "norm2": (C,), p + "attn.qkv": (3 * C, C), p + "attn.proj": (C, C), p + "mlp.fc1": (hidden, C),
                         p + "mlp.fc2": (C, hidden), p + "conv_block.cab.0": (Cc, C, 3, 3), p + "conv_block.cab.2": (C, Cc, 3, 3),
                         p + "conv_block.cab.3.attention.1": (Cs, C, 1, 1), p + "conv_block.cab.3.attention.3": (C, Cs, 1, 1)})
            tables[p + "attn.relative_position_bias_table"] = (SA_ROWS, heads[i])
        for name, shape in tables.items():
            if name not in sd or tuple(sd[name].shape) != shape:
                raise UpscalerFormatError(f"hat: {name} is missing or not {shape}")
    for name, shape in want.items():
        w, b = sd.get(name + ".weight"), sd.get(name + ".bias")
        if w is None or b is None:
            raise UpscalerFormatError(f"hat: the checkpoint has no {name}.weight / .bias")
        if tuple(w.shape) != shape or tuple(b.shape) != shape[:1]:
            raise UpscalerFormatError(f"hat: {name}.weight is {tuple(w.shape)}, expected {shape}")
    known = {n + s for n in want for s in (".weight", ".bias")}
    extra = sorted(k for k in ks if k not in known and not _IGNORED.search(k) and not k.endswith("relative_position_bias_table"))
    if extra:
        raise UpscalerFormatError(f"hat: unexpected key {extra[0]!r} (+{len(extra) - 1} more): not a plain HAT")
    return dict(embed_dim=C, depths=depths, heads=heads, mlp_hidden=hidden, ocab_hidden=hid2, compress=Cc, squeeze=Cs, num_feat=nf, scale=scale)


class HAT:
    """The network on one device, with SwinIR's and RRDBNet's interface: call it with NHWC bf16 RGB in [0, 1] -> NHWC bf16 at `scale` times
    the size; upscale_uint8 / upscale_uint8_device wrap the value range the same way."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda:0"):
        sd = unwrap(state_dict)
        g = self.geometry = infer_geometry(sd)
        self.scale, self.C, self.nf = g["scale"], g["embed_dim"], g["num_feat"]
        self.Cp, self.Cm = _up(self.C, 64), _up(g["compress"], 32)
        self.Fp, self.Fo = _up(g["mlp_hidden"], 128), _up(g["ocab_hidden"], 128)
        self.device = dev = torch.device(device)
        C, Cp, Cm, nf, Cs = self.C, self.Cp, self.Cm, self.nf, g["squeeze"]
        self.w = w = {}
        self.index_sa = _index(sd, "relative_position_index_SA", index_sa, SA_ROWS, WINDOW ** 2).to(dev)
        self.index_oca = _index(sd, "relative_position_index_OCA", index_oca, OCA_ROWS, (WINDOW + 2 * OVERLAP) ** 2).to(dev)

        def conv(name, cin_p, cout_p):  # Conv2d [Cout, Cin, 3, 3] -> the kernel's [cout_p, 3, 3, cin_p]
            wt, b = sd[name + ".weight"], sd[name + ".bias"]
            w2 = torch.zeros(cout_p, 3, 3, cin_p, dtype=torch.bfloat16)
            w2[: wt.shape[0], :, :, : wt.shape[1]] = wt.permute(0, 2, 3, 1).to(torch.bfloat16)
            w[name] = (w2.to(dev), _pad1(b, cout_p).to(dev))

        def norm(name):
            w[name] = (_pad1(sd[name + ".weight"], _up(C, 8)).to(dev), _pad1(sd[name + ".bias"], _up(C, 8)).to(dev))

        def linear(name, rows, cols):
            w[name] = (_pad2(sd[name + ".weight"], rows, cols).to(dev), _pad1(sd[name + ".bias"], rows).to(dev))

        conv("conv_first", 16, Cp), conv("conv_after_body", Cp, Cp), conv("conv_before_upsample.0", Cp, _up(nf, 32))
        norm("patch_embed.norm"), norm("norm")
        conv("upsample.0", nf, 4 * nf), conv("conv_last", nf, 32)
        if self.scale == 4:
            conv("upsample.2", nf, 4 * nf)
        for i, (depth, heads) in enumerate(zip(g["depths"], g["heads"])):
            conv(f"layers.{i}.conv", Cp, Cp)
            Ka, Nq = _up(heads * HEAD_PAD, 64), _up(3 * heads * HEAD_PAD, 128)
            hx = _head_index(C, heads)
            rows = torch.cat([s * heads * HEAD_PAD + hx for s in range(3)])

            def attention(p, a):  # p + a + "qkv" / "proj": rows of qkv and columns of proj moved to the head-padded layout
                wq, bq = torch.zeros(Nq, Cp, dtype=torch.bfloat16), torch.zeros(Nq, dtype=torch.bfloat16)
                wq[rows, :C], bq[rows] = sd[p + a + "qkv.weight"].to(torch.bfloat16), sd[p + a + "qkv.bias"].to(torch.bfloat16)
                wp = torch.zeros(Cp, Ka, dtype=torch.bfloat16)
                wp[:C, hx] = sd[p + a + "proj.weight"].to(torch.bfloat16)
                w[p + a + "qkv"] = (wq.to(dev), bq.to(dev))
                w[p + a + "proj"] = (wp.to(dev), _pad1(sd[p + a + "proj.bias"], Cp).to(dev))
                w[p + "table"] = sd[p + a + "relative_position_bias_table"].float().contiguous().to(dev)
                norm(p + "norm1"), norm(p + "norm2")

            for j in range(depth):
                p = f"layers.{i}.residual_group.blocks.{j}."
                attention(p, "attn.")
                linear(p + "mlp.fc1", self.Fp, Cp), linear(p + "mlp.fc2", Cp, self.Fp)
                conv(p + "conv_block.cab.0", Cp, Cm), conv(p + "conv_block.cab.2", Cm, Cp)
                w1, b1, w2, b2 = torch.zeros(Cs, Cp), sd[p + "conv_block.cab.3.attention.1.bias"].float(), torch.zeros(Cp, Cs), torch.zeros(Cp)
                w1[:, :C] = sd[p + "conv_block.cab.3.attention.1.weight"].float().view(Cs, C)
                w2[:C], b2[:C] = sd[p + "conv_block.cab.3.attention.3.weight"].float().view(C, Cs), sd[p + "conv_block.cab.3.attention.3.bias"].float()
                w[p + "gate"] = tuple(t.contiguous().to(dev) for t in (w1, b1, w2, b2))
            p = f"layers.{i}.residual_group.overlap_attn."
            attention(p, "")
            linear(p + "mlp.fc1", self.Fo, Cp), linear(p + "mlp.fc2", Cp, self.Fo)
        self.ones = torch.ones(Cp, dtype=torch.bfloat16, device=dev)
        self.mean = torch.tensor(MEAN, dtype=torch.float32, device=dev)

    # ---- limits ----------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def padded_size(H: int, W: int):
        return _up(H, WINDOW), _up(W, WINDOW)

    def memory_estimate(self, B: int, H: int, W: int) -> int:
        """bytes of activations the forward holds at its peak for a [B, H, W, 3] input: the larger of the trunk (the features, the group's
        input and output, the normed rows, two token buffers, proj's and CAB's outputs, CAB's hidden rows, qkv, the attention output, the
        MLP's hidden rows) and the tail (each upsample convolution's output next to its shuffled copy, and the RGB)"""
        Hp, Wp = self.padded_size(H, W)
        px, heads = B * Hp * Wp, max(self.geometry["heads"])
        trunk = px * 2 * (8 * self.Cp + self.Cm + 4 * heads * HEAD_PAD + 192 + max(self.Fp, self.Fo) + 16)
        tail = px * 2 * (self.Cp + self.nf + (8 if self.scale == 2 else 5 + 32) * self.nf + self.scale ** 2 * 8)
        return max(trunk, tail)

    def check_input(self, B: int, H: int, W: int) -> None:
        """refuse, by name, what the padding, the kernels' addressing or the device's free memory cannot take"""
        from fluxmi import ops

        Hp, Wp = self.padded_size(H, W)
        if B < 1 or H < 1 or W < 1 or Hp - H >= H or Wp - W >= W:
            raise ValueError(f"upscaler: HAT reflect-pads H, W to multiples of {WINDOW}, which needs each side above its padding "
                             f"(>= {WINDOW // 2 + 1}, or {WINDOW}), got {B} x {H} x {W}")
        tiles = -(-(Hp * self.scale) // ops.CONV_DENSE_TILE)
        if B > 65535 or tiles > 65535:
            raise ValueError(f"upscaler: B={B} images / {tiles} tile rows exceed the kernels' launch grid (65535 each)")
        if self.device.type == "cuda":
            free = torch.cuda.mem_get_info(self.device)[0] + torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
            need = self.memory_estimate(B, H, W)
            if need > free:
                raise ValueError(f"upscaler: {B} x {H} x {W} needs about {need / 2 ** 30:.1f} GiB of activations, {free / 2 ** 30:.1f} GiB are "
                                 "free; the network is not tiled: send a smaller image")

    # ---- forward ---------------------------------------------------------------------------------------------------------------------
    def _conv(self, name, x, out, act=False, slope=0.01, r1=None):
        """fluxmi_conv3x3_dense in windows of at most 64 output channels; `out` may be narrower than the packed weight (conv_last: 3 of 32)"""
        from fluxmi import ops

        w2, b2 = self.w[name]
        for c0 in range(0, out.shape[-1], 64):
            n = min(64, out.shape[-1] - c0)
            n32 = _up(n, 32)
            ops.conv3x3_dense(x, w2[c0:c0 + n32], b2[c0:c0 + n32], out[..., c0:c0 + n], r1=None if r1 is None else r1[..., c0:c0 + n], a1=1.0,
                              slope=slope, act=act)
        return out

    @torch.inference_mode()
    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        from fluxmi import _lib, ops

        if x.ndim != 4 or x.shape[-1] != 3 or x.dtype != torch.bfloat16:
            raise ValueError(f"upscaler: expected NHWC bf16 RGB [B, H, W, 3], got {tuple(x.shape)} {x.dtype}")
        B, H0, W0, _ = x.shape
        self.check_input(B, H0, W0)
        g, dev, C, Cp, nf, s = self.geometry, self.device, self.C, self.Cp, self.nf, self.scale
        H, W = self.padded_size(H0, W0)
        xn = (x.to(dev).float() - self.mean).permute(0, 3, 1, 2)
        xn = F.pad(xn, (0, W - W0, 0, H - H0), mode="reflect").permute(0, 2, 3, 1)
        new = lambda h, w, c: torch.empty(B, h, w, c, dtype=torch.bfloat16, device=dev)  # noqa: E731
        xin = torch.zeros(B, H, W, 16, dtype=torch.bfloat16, device=dev)
        xin[..., :3] = xn.to(torch.bfloat16)
        M = B * H * W
        img = lambda t: t.view(B, H, W, t.shape[-1])  # noqa: E731
        feat = self._conv("conv_first", xin, new(H, W, Cp))
        t = ops.channel_norm(feat.view(M, Cp), *self.w["patch_embed.norm"], C, LN_EPS)
        h = torch.zeros(M, Cp, dtype=torch.bfloat16, device=dev)  # the normed rows; channel_norm writes [0, C rounded up to 8), the rest stays zero
        mid, tok, pa, cab = (torch.empty(M, Cp, dtype=torch.bfloat16, device=dev) for _ in range(4))
        cm = new(H, W, self.Cm)
        hid = torch.empty(M, max(self.Fp, self.Fo), dtype=torch.bfloat16, device=dev)

        def mlp(p, F_):  # tok = mid + fc2(gelu(fc1(norm2(mid))))
            ops.channel_norm(mid, *self.w[p + "norm2"], C, LN_EPS, out=h)
            ops.linear(h, *self.w[p + "mlp.fc1"], out=hid[:, :F_])
            ops.unary(hid[:, :F_], "gelu", out=hid[:, :F_])
            ops.linear(hid[:, :F_], *self.w[p + "mlp.fc2"], epilogue=_lib.EPI_GATE_RESID, gate=self.ones, resid=mid, out=tok)

        for i, (depth, heads) in enumerate(zip(g["depths"], g["heads"])):
            Cw, Ka, Nq = heads * HEAD_PAD, _up(heads * HEAD_PAD, 64), _up(3 * heads * HEAD_PAD, 128)
            qkv, att = torch.empty(M, Nq, dtype=torch.bfloat16, device=dev), torch.zeros(M, Ka, dtype=torch.bfloat16, device=dev)
            scale = float((C // heads) ** -0.5)
            # the group's input `res` is its residual and is never written: a block reads cur (res, then tok), writes mid, then tok
            res, cur = t, t
            for j in range(depth):
                p = f"layers.{i}.residual_group.blocks.{j}."
                ops.channel_norm(cur, *self.w[p + "norm1"], C, LN_EPS, out=h)
                ops.linear(h, *self.w[p + "attn.qkv"], out=qkv)
                ops.window_attention16(img(qkv)[..., :3 * Cw], self.w[p + "table"], self.index_sa, heads, (j % 2) * (WINDOW // 2), 0, scale,
                                       out=img(att)[..., :Cw], check_index=False)
                ops.linear(att, *self.w[p + "attn.proj"], out=pa)
                self._conv(p + "conv_block.cab.0", img(h), cm)
                ops.unary(cm, "gelu", out=cm)
                self._conv(p + "conv_block.cab.2", cm, img(cab))
                ops.channel_combine(img(cur), img(pa), img(cab), ops.channel_mean(img(cab)), *self.w[p + "gate"], CONV_SCALE, out=img(mid))
                mlp(p, self.Fp)
                cur = tok
            p = f"layers.{i}.residual_group.overlap_attn."
            ops.channel_norm(cur, *self.w[p + "norm1"], C, LN_EPS, out=h)
            ops.linear(h, *self.w[p + "qkv"], out=qkv)
            ops.window_attention16(img(qkv)[..., :3 * Cw], self.w[p + "table"], self.index_oca, heads, 0, OVERLAP, scale,
                                   out=img(att)[..., :Cw], check_index=False)
            ops.linear(att, *self.w[p + "proj"], epilogue=_lib.EPI_GATE_RESID, gate=self.ones, resid=cur, out=mid)
            mlp(p, self.Fo)
            t = self._conv(f"layers.{i}.conv", img(tok), new(H, W, Cp), r1=img(res)).view(M, Cp)
        ops.channel_norm(t, *self.w["norm"], C, LN_EPS, out=h)
        trunk = self._conv("conv_after_body", img(h), new(H, W, Cp), r1=feat)
        del feat, t, h, mid, tok, pa, cab, cm, hid, qkv, att, res, cur
        y = self._conv("conv_before_upsample.0", trunk, new(H, W, nf), act=True, slope=0.01)
        del trunk
        for n in ("upsample.0", "upsample.2")[: s // 2]:  # conv nf -> 4 nf, PixelShuffle(2): channel c * 4 + 2 i + j goes to pixel (2 y + i, 2 x + j)
            Hy, Wy = y.shape[1:3]
            y = self._conv(n, y, new(Hy, Wy, 4 * nf)).view(B, Hy, Wy, nf, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * Hy, 2 * Wy, nf)
        rgb = self._conv("conv_last", y, new(s * H, s * W, 8)[..., :3])
        return (rgb[:, : s * H0, : s * W0].float() + self.mean).to(torch.bfloat16)

    def _uint8(self, px: torch.Tensor) -> torch.Tensor:
        if px.dtype != torch.uint8 or px.ndim != 4 or px.shape[-1] != 3:
            raise ValueError(f"upscaler: expected uint8 [B, H, W, 3], got {tuple(px.shape)} {px.dtype}")
        y = self(px.to(self.device).float().div(255.0).to(torch.bfloat16))
        return y.float().clamp(0.0, 1.0).mul(255.0).round().to(torch.uint8).contiguous()

    def upscale_uint8(self, px: torch.Tensor) -> torch.Tensor:
        """uint8 [B, H, W, 3] (any device) -> uint8 [B, scale H, scale W, 3] on the host"""
        return self._uint8(px).cpu()

    def upscale_uint8_device(self, px: torch.Tensor) -> torch.Tensor:
        """upscale_uint8's arithmetic with the result left on the network's device (contiguous): what the native JPEG encoder reads"""
        return self._uint8(px)
