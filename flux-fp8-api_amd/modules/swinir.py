"""SwinIR -- the Swin-transformer restoration network behind the "SwinIR 4x" real-world upscalers (003_realSR_BSRGAN_DFO*_SwinIR-M / L
x4 / x2 GAN) -- on fluxmi_window_attention (csrc/window_attention.hip).  The definition is KAIR's models/network_swinir.py:

  x     = (x - mean) * img_range, reflect-padded to multiples of the window (8);  mean = (0.4488, 0.4371, 0.4040), img_range = 1
  feat  = conv_first(x)                                                      3 -> C (embed_dim)
  body  : t = LayerNorm(feat) (patch_embed.norm);  RSTB^n;  LayerNorm (norm);  trunk = conv_after_body(t) + feat
  RSTB  : t + conv(blocks(t));  conv = one 3x3 ("1conv") or 3x3 C -> C/4, LeakyReLU 0.2, 1x1, LeakyReLU 0.2, 3x3 C/4 -> C ("3conv")
  block : t = t + proj(window_attention(qkv(norm1(t))));  t = t + fc2(gelu(fc1(norm2(t))))        shift 0 in even blocks, 4 in odd ones,
          scale = head_dim^-1/2, the exact (erf) GELU, LayerNorm eps 1e-5
  out   = conv_last(lrelu_0.2(conv_hr(lrelu_0.2(conv_up2(up2x(lrelu_0.2(conv_up1(up2x(lrelu_0.01(conv_before_upsample(trunk)))))))))))
          ("nearest+conv"; x2 has no conv_up2), + mean, cropped to scale * (H, W)

On libfluxmi: activations are NHWC bf16 rows of Cp = C rounded up to 64 channels (180 -> 192, 240 -> 256) whose pad channels are held at
zero -- zero weight rows / columns keep them there through every launch, so the padded network computes exactly the unpadded one.  LayerNorm
over the C real channels is fluxmi_channel_norm; qkv / proj / fc1 / fc2 are the bf16 GEMM (ops.linear), the two residual sums its
gate * y + x epilogue with a ones gate, as in the text towers; GELU is fluxmi_unary.  The rows of the fused qkv weight are permuted and
zero-padded so that every head is 32 columns wide (a 30-wide head is followed by two zeros), the layout fluxmi_window_attention reads; the
partition, both cyclic shifts and the reverse are address arithmetic inside that one launch; proj's columns are permuted to match.
Convolutions run on fluxmi_conv3x3_dense in channel windows of at most 64 outputs, the RSTB's residual as its r1, LeakyReLU and the nearest
2x (upsample = 2) folded in.  The 1x1 of "3conv" runs there too, as a 3x3 whose eight outer taps are zero (the GEMM has no LeakyReLU
epilogue; the layer is C/4 -> C/4).  Every launch rounds to bf16 once.

Geometry (embed_dim, depths, heads per layer, the MLP width, 1conv / 3conv, the upscale) is read from the checkpoint and every expected
tensor is checked by name and shape; keys may be wrapped in params_ema / params.  The relative_position_index and attn_mask buffers are
ignored: both are functions of the geometry, and the mask is recomputed per input size, as SwinIR itself does.  Supported: window 8,
head_dim <= 32, C <= 256, "nearest+conv" at x2 / x4.  Refused by name: pixelshuffle, pixelshuffledirect, the upscale-1 denoise / JPEG models,
windows 7 / 16, ape, Swin2SR, HAT.  The key layout is written from the public code; no real checkpoint has been loaded here, and image
quality is unverified (synthetic weights only).
"""
from __future__ import annotations

import re
from typing import Dict

import torch
import torch.nn.functional as F

from modules.upscaler import UpscalerFormatError

WINDOW, HEAD_PAD = 8, 32
MEAN = (0.4488, 0.4371, 0.4040)
LN_EPS = 1e-5
_BLOCK = re.compile(r"^layers\.(\d+)\.residual_group\.blocks\.(\d+)\.")
_IGNORED = re.compile(r"(\.attn\.relative_position_index|\.attn_mask)$")


def _up(n: int, m: int) -> int:
    return -(-n // m) * m


def unwrap(sd: dict) -> dict:
    for wrap in ("params_ema", "params"):
        if wrap in sd and isinstance(sd[wrap], dict):
            return sd[wrap]
    return sd


def is_swin_family(sd: dict) -> bool:
    """does the (possibly wrapped) state dict look like SwinIR or one of its descendants: read_upscaler's dispatch"""
    return any(".residual_group." in k or k.startswith("patch_embed.") for k in unwrap(sd))


def _conv_kind(sd, name: str) -> str:
    if name + ".weight" in sd:
        return "1conv"
    if name + ".0.weight" in sd and name + ".4.weight" in sd:
        return "3conv"
    raise UpscalerFormatError(f"swinir: the checkpoint has neither {name}.weight (1conv) nor {name}.0 / .2 / .4 (3conv)")


def infer_geometry(sd: Dict[str, torch.Tensor]) -> dict:
    """unwrapped KAIR keys -> dict(embed_dim, depths, heads, mlp_hidden, resi, after_body, num_feat, scale); every expected tensor is checked
    by name and shape, anything else is refused by name"""
    ks = list(sd)
    has = lambda s: any(s in k for k in ks)  # noqa: E731
    if has("logit_scale") or has("cpb_mlp"):
        raise UpscalerFormatError("swinir: this checkpoint is a Swin2SR network (logit_scale / cpb_mlp: cosine attention with a learned position MLP); only SwinIR is supported")
    if has("overlap_attn") or has("conv_block.cab") or has("attn_blocks"):
        raise UpscalerFormatError("swinir: this checkpoint is a HAT network (channel attention / overlapping cross-attention blocks); only SwinIR is supported")
    if "absolute_pos_embed" in sd:
        raise UpscalerFormatError("swinir: this checkpoint uses ape (an absolute position embedding of a fixed image size); not supported")
    if "conv_first.weight" not in sd or not any(_BLOCK.match(k) for k in ks):
        raise UpscalerFormatError("swinir: not a SwinIR checkpoint (no conv_first / layers.*.residual_group.blocks.*)")
    C = int(sd["conv_first.weight"].shape[0])
    if "upsample.0.weight" in sd:
        kind = "pixelshuffle" if "conv_before_upsample.0.weight" in sd else "pixelshuffledirect"
        raise UpscalerFormatError(f"swinir: this checkpoint reconstructs with {kind} (the classical / lightweight SR models); only 'nearest+conv' "
                                  "(the real-world x2 / x4 models) is supported")
    if "conv_before_upsample.0.weight" not in sd:
        raise UpscalerFormatError("swinir: this checkpoint has no upsampler (an upscale-1 denoise / JPEG model: conv_last reads embed_dim); not supported")
    depths = {}
    for k in ks:
        m = _BLOCK.match(k)
        if m:
            i, j = int(m.group(1)), int(m.group(2))
            depths[i] = max(depths.get(i, 0), j + 1)
    n_layers = 1 + max(depths)
    if sorted(depths) != list(range(n_layers)):
        raise UpscalerFormatError(f"swinir: layers {sorted(depths)} are not 0..{n_layers - 1}")
    depths = [depths[i] for i in range(n_layers)]
    heads, hidden = [], None
    for i in range(n_layers):
        t = sd.get(f"layers.{i}.residual_group.blocks.0.attn.relative_position_bias_table")
        if t is None or t.ndim != 2:
            raise UpscalerFormatError(f"swinir: layers.{i} has no relative_position_bias_table")
        side = {169: 7, 961: 16}.get(int(t.shape[0]))
        if int(t.shape[0]) != (2 * WINDOW - 1) ** 2:
            raise UpscalerFormatError(f"swinir: the bias table has {t.shape[0]} rows" + (f" (window {side})" if side else "") +
                                      f"; only window {WINDOW} ({(2 * WINDOW - 1) ** 2} rows) is supported")
        heads.append(int(t.shape[1]))
        if C % heads[-1] or C // heads[-1] > HEAD_PAD:
            raise UpscalerFormatError(f"swinir: layers.{i}: embed_dim {C} over {heads[-1]} heads: head_dim must divide and be <= {HEAD_PAD}")
    hidden = int(sd["layers.0.residual_group.blocks.0.mlp.fc1.weight"].shape[0]) if "layers.0.residual_group.blocks.0.mlp.fc1.weight" in sd else 0
    if _up(C, 64) > 256:
        raise UpscalerFormatError(f"swinir: embed_dim {C} pads to {_up(C, 64)} channels; fluxmi_conv3x3_dense reads at most 256")
    resi, after = _conv_kind(sd, "layers.0.conv"), _conv_kind(sd, "conv_after_body")
    nf = int(sd["conv_before_upsample.0.weight"].shape[0])
    if nf % 16 or not 16 <= nf <= 64:
        raise UpscalerFormatError(f"swinir: num_feat={nf}: the reconstruction convolutions take a multiple of 16 in 16..64")
    scale = 4 if "conv_up2.weight" in sd else 2
    want = {"conv_first": (C, 3, 3, 3), "conv_before_upsample.0": (nf, C, 3, 3), "conv_up1": (nf, nf, 3, 3), "conv_hr": (nf, nf, 3, 3),
            "conv_last": (3, nf, 3, 3), "patch_embed.norm": (C,), "norm": (C,)}
    if scale == 4:
        want["conv_up2"] = (nf, nf, 3, 3)

    def conv_names(name, kind):
        q = C // 4
        return {name: (C, C, 3, 3)} if kind == "1conv" else {name + ".0": (q, C, 3, 3), name + ".2": (q, q, 1, 1), name + ".4": (C, q, 3, 3)}

    want.update(conv_names("conv_after_body", after))
    for i in range(n_layers):
        want.update(conv_names(f"layers.{i}.conv", resi))
        for j in range(depths[i]):
            p = f"layers.{i}.residual_group.blocks.{j}."
            want.update({p + "norm1": (C,), p + "norm2": (C,), p + "attn.qkv": (3 * C, C), p + "attn.proj": (C, C),
                         p + "mlp.fc1": (hidden, C), p + "mlp.fc2": (C, hidden)})
            t = sd.get(p + "attn.relative_position_bias_table")
            if t is None or tuple(t.shape) != ((2 * WINDOW - 1) ** 2, heads[i]):
                raise UpscalerFormatError(f"swinir: {p}attn.relative_position_bias_table is missing or not {((2 * WINDOW - 1) ** 2, heads[i])}")
    for name, shape in want.items():
        w, b = sd.get(name + ".weight"), sd.get(name + ".bias")
        if w is None or b is None:
            raise UpscalerFormatError(f"swinir: the checkpoint has no {name}.weight / .bias")
        if tuple(w.shape) != shape or tuple(b.shape) != shape[:1]:
            raise UpscalerFormatError(f"swinir: {name}.weight is {tuple(w.shape)}, expected {shape}")
    known = {n + s for n in want for s in (".weight", ".bias")}
    extra = sorted(k for k in ks if k not in known and not _IGNORED.search(k) and not k.endswith("attn.relative_position_bias_table"))
    if extra:
        raise UpscalerFormatError(f"swinir: unexpected key {extra[0]!r} (+{len(extra) - 1} more): not a plain SwinIR")
    return dict(embed_dim=C, depths=depths, heads=heads, mlp_hidden=hidden, resi=resi, after_body=after, num_feat=nf, scale=scale)


def _pad2(w: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    out = torch.zeros(rows, cols, dtype=torch.bfloat16)
    out[: w.shape[0], : w.shape[1]] = w.to(torch.bfloat16)
    return out


def _pad1(b: torch.Tensor, n: int) -> torch.Tensor:
    out = torch.zeros(n, dtype=torch.bfloat16)
    out[: b.shape[0]] = b.to(torch.bfloat16)
    return out


def _head_index(C: int, heads: int) -> torch.Tensor:
    """position of channel h * hd + d in the head-padded layout: h * 32 + d"""
    hd = C // heads
    c = torch.arange(C)
    return (c // hd) * HEAD_PAD + c % hd


class SwinIR:
    """The network on one device, with RRDBNet's interface (modules/upscaler.py): call it with NHWC bf16 RGB in [0, 1] -> NHWC bf16 at
    `scale` times the size; upscale_uint8 / upscale_uint8_device wrap the value range the same way."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda:0"):
        sd = unwrap(state_dict)
        g = self.geometry = infer_geometry(sd)
        self.scale, self.C, self.nf = g["scale"], g["embed_dim"], g["num_feat"]
        self.Cp, self.Cq, self.Fp = _up(self.C, 64), _up(self.C // 4, 32), _up(g["mlp_hidden"], 128)
        self.device = dev = torch.device(device)
        C, Cp, Cq, nf = self.C, self.Cp, self.Cq, self.nf
        self.w = w = {}

        def conv(name, cin_p, cout_p):  # Conv2d [Cout, Cin, k, k] -> the kernel's [cout_p, 3, 3, cin_p]; a 1x1 becomes the centre tap
            wt, b = sd[name + ".weight"], sd[name + ".bias"]
            co, ci, k = wt.shape[0], wt.shape[1], wt.shape[2]
            w2 = torch.zeros(cout_p, 3, 3, cin_p, dtype=torch.bfloat16)
            lo = (3 - k) // 2
            w2[:co, lo:lo + k, lo:lo + k, :ci] = wt.permute(0, 2, 3, 1).to(torch.bfloat16)
            w[name] = (w2.to(dev), _pad1(b, cout_p).to(dev))

        def body_conv(name, kind):
            if kind == "1conv":
                conv(name, Cp, Cp)
            else:
                conv(name + ".0", Cp, Cq), conv(name + ".2", Cq, Cq), conv(name + ".4", Cq, Cp)

        def norm(name):
            w[name] = (_pad1(sd[name + ".weight"], _up(C, 8)).to(dev), _pad1(sd[name + ".bias"], _up(C, 8)).to(dev))

        conv("conv_first", 16, Cp)
        norm("patch_embed.norm"), norm("norm")
        body_conv("conv_after_body", g["after_body"])
        conv("conv_before_upsample.0", Cp, _up(nf, 32))
        for n in ("conv_up1", "conv_up2", "conv_hr"):
            if n + ".weight" in sd:
                conv(n, nf, _up(nf, 32))
        conv("conv_last", nf, 32)
        for i, (depth, heads) in enumerate(zip(g["depths"], g["heads"])):
            body_conv(f"layers.{i}.conv", g["resi"])
            Ka, Nq = _up(heads * HEAD_PAD, 64), _up(3 * heads * HEAD_PAD, 128)
            hx = _head_index(C, heads)
            rows = torch.cat([s * heads * HEAD_PAD + hx for s in range(3)])
            for j in range(depth):
                p = f"layers.{i}.residual_group.blocks.{j}."
                norm(p + "norm1"), norm(p + "norm2")
                wq, bq = torch.zeros(Nq, Cp, dtype=torch.bfloat16), torch.zeros(Nq, dtype=torch.bfloat16)
                wq[rows, :C], bq[rows] = sd[p + "attn.qkv.weight"].to(torch.bfloat16), sd[p + "attn.qkv.bias"].to(torch.bfloat16)
                wp = torch.zeros(Cp, Ka, dtype=torch.bfloat16)
                wp[:C, hx] = sd[p + "attn.proj.weight"].to(torch.bfloat16)
                w[p + "attn.qkv"] = (wq.to(dev), bq.to(dev))
                w[p + "attn.proj"] = (wp.to(dev), _pad1(sd[p + "attn.proj.bias"], Cp).to(dev))
                w[p + "mlp.fc1"] = (_pad2(sd[p + "mlp.fc1.weight"], self.Fp, Cp).to(dev), _pad1(sd[p + "mlp.fc1.bias"], self.Fp).to(dev))
                w[p + "mlp.fc2"] = (_pad2(sd[p + "mlp.fc2.weight"], Cp, self.Fp).to(dev), _pad1(sd[p + "mlp.fc2.bias"], Cp).to(dev))
                w[p + "table"] = sd[p + "attn.relative_position_bias_table"].float().contiguous().to(dev)
        self.ones = torch.ones(Cp, dtype=torch.bfloat16, device=dev)
        self.mean = torch.tensor(MEAN, dtype=torch.float32, device=dev)

    # ---- limits ----------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def padded_size(H: int, W: int):
        return _up(H, WINDOW), _up(W, WINDOW)

    def memory_estimate(self, B: int, H: int, W: int) -> int:
        """bytes of activations the forward holds at its peak for a [B, H, W, 3] input: the larger of the trunk (the features, the layer's
        input, two token buffers, the normed rows, qkv, the attention output, the MLP's hidden rows) and the tail (conv_up2's and conv_hr's
        full-resolution outputs and the padded RGB)"""
        Hp, Wp = self.padded_size(H, W)
        px, heads = B * Hp * Wp, max(self.geometry["heads"])
        trunk = px * 2 * (5 * self.Cp + 4 * heads * HEAD_PAD + 192 + self.Fp + 16)
        tail = px * 2 * (self.Cp + 5 * self.nf + self.scale ** 2 * (2 * self.nf + 8))
        return max(trunk, tail)

    def check_input(self, B: int, H: int, W: int) -> None:
        """refuse, by name, what the padding, the kernels' addressing or the device's free memory cannot take"""
        from fluxmi import ops

        Hp, Wp = self.padded_size(H, W)
        if B < 1 or H < 1 or W < 1 or Hp - H >= H or Wp - W >= W:
            raise ValueError(f"upscaler: SwinIR reflect-pads H, W to multiples of {WINDOW}, which needs each side above its padding "
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
    def _conv(self, name, x, out, act=False, slope=0.2, upsample=1, r1=None):
        """fluxmi_conv3x3_dense in windows of at most 64 output channels; `out` may be narrower than the packed weight (conv_last: 3 of 32)"""
        from fluxmi import ops

        w2, b2 = self.w[name]
        for c0 in range(0, out.shape[-1], 64):
            n = min(64, out.shape[-1] - c0)
            n32 = _up(n, 32)
            ops.conv3x3_dense(x, w2[c0:c0 + n32], b2[c0:c0 + n32], out[..., c0:c0 + n], r1=None if r1 is None else r1[..., c0:c0 + n], a1=1.0,
                              slope=slope, act=act, upsample=upsample)
        return out

    def _body_conv(self, name, kind, x, out, r1):
        if kind == "1conv":
            return self._conv(name, x, out, r1=r1)
        B, H, W, _ = x.shape
        a, b = (torch.empty(B, H, W, self.Cq, dtype=torch.bfloat16, device=x.device) for _ in range(2))
        self._conv(name + ".0", x, a, act=True)
        self._conv(name + ".2", a, b, act=True)
        return self._conv(name + ".4", b, out, r1=r1)

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
        feat = self._conv("conv_first", xin, new(H, W, Cp))
        t = ops.channel_norm(feat.view(M, Cp), *self.w["patch_embed.norm"], C, LN_EPS)
        h = torch.zeros(M, Cp, dtype=torch.bfloat16, device=dev)  # the normed rows; channel_norm writes [0, C rounded up to 8), the rest stays zero
        mid, tok = (torch.empty(M, Cp, dtype=torch.bfloat16, device=dev) for _ in range(2))
        hid = torch.empty(M, self.Fp, dtype=torch.bfloat16, device=dev)
        for i, (depth, heads) in enumerate(zip(g["depths"], g["heads"])):
            Cw, Ka, Nq = heads * HEAD_PAD, _up(heads * HEAD_PAD, 64), _up(3 * heads * HEAD_PAD, 128)
            qkv, att = torch.empty(M, Nq, dtype=torch.bfloat16, device=dev), torch.zeros(M, Ka, dtype=torch.bfloat16, device=dev)
            scale = float((C // heads) ** -0.5)
            res, cur = t, t
            for j in range(depth):
                p = f"layers.{i}.residual_group.blocks.{j}."
                ops.channel_norm(cur, *self.w[p + "norm1"], C, LN_EPS, out=h)
                ops.linear(h, *self.w[p + "attn.qkv"], out=qkv)
                ops.window_attention(qkv.view(B, H, W, Nq)[..., :3 * Cw], self.w[p + "table"], heads, (j % 2) * (WINDOW // 2), scale,
                                     out=att.view(B, H, W, Ka)[..., :Cw])
                # the layer's input `res` is the RSTB's residual and is never written: a block reads cur (res, then tok), writes mid, then tok
                ops.linear(att, *self.w[p + "attn.proj"], epilogue=_lib.EPI_GATE_RESID, gate=self.ones, resid=cur, out=mid)
                ops.channel_norm(mid, *self.w[p + "norm2"], C, LN_EPS, out=h)
                ops.linear(h, *self.w[p + "mlp.fc1"], out=hid)
                ops.unary(hid, "gelu", out=hid)
                ops.linear(hid, *self.w[p + "mlp.fc2"], epilogue=_lib.EPI_GATE_RESID, gate=self.ones, resid=mid, out=tok)
                cur = tok
            t = self._body_conv(f"layers.{i}.conv", g["resi"], cur.view(B, H, W, Cp), new(H, W, Cp), res.view(B, H, W, Cp)).view(M, Cp)
        ops.channel_norm(t, *self.w["norm"], C, LN_EPS, out=h)
        trunk = self._body_conv("conv_after_body", g["after_body"], h.view(B, H, W, Cp), new(H, W, Cp), feat)
        del feat, t, h, mid, tok, hid, qkv, att, res, cur
        y = self._conv("conv_before_upsample.0", trunk, new(H, W, nf), act=True, slope=0.01)
        del trunk
        y = self._conv("conv_up1", y, new(2 * H, 2 * W, nf), act=True, upsample=2)
        if s == 4:
            y = self._conv("conv_up2", y, new(4 * H, 4 * W, nf), act=True, upsample=2)
        y = self._conv("conv_hr", y, new(s * H, s * W, nf), act=True)
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
