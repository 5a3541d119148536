"""RRDBNet -- the network behind ESRGAN, Real-ESRGAN x4plus / x2plus, 4x-UltraSharp and most community upscalers -- on
fluxmi_conv3x3_dense (csrc/upscaler.hip).  The definition is BasicSR's / Real-ESRGAN's (basicsr/archs/rrdbnet_arch.py):

  feat  = conv_first(x)                                    x: RGB in [0, 1]; scale 2 / 1: pixel_unshuffle(x, 2 / 4) first (12 / 48 channels)
  RDB   : x_k = lrelu_0.2(conv_k(cat(x, x_1 .. x_{k-1}))), k = 1..4;  out = x + 0.2 conv_5(cat(x, x_1 .. x_4))
  RRDB  : out = x + 0.2 rdb3(rdb2(rdb1(x)))
  trunk = conv_body(RRDB^n(feat)) + feat
  out   = conv_last(lrelu(conv_hr(lrelu(conv_up2(up2x(lrelu(conv_up1(up2x(trunk)))))))))          up2x = nearest

Activations are NHWC bf16.  An RDB is FIVE launches on one [B, H, W, nf + 4 gc] buffer: conv k reads the channel window [0, nf + (k-1) gc)
and writes [nf + (k-1) gc, nf + k gc) in place -- no torch.cat; conv 5 writes channels [0, nf) of the NEXT block's buffer with the RDB
residual as r1 and, in an RRDB's third RDB, the RRDB residual as r2 of the same launch.  The nearest upsamples are folded into conv_up1 / 2
(upsample = 2).  The 3 (12) input channels are zero-padded to 16; conv_last runs at Cout = 3.  Every launch rounds to bf16 once.

Checkpoints: BasicSR "new" keys (conv_first, body.{i}.rdb{j}.conv{k}, conv_body, conv_up1 / 2, conv_hr, conv_last; possibly under
params_ema / params) and the original ESRGAN "old arch" x4 keys (model.0, model.1.sub.{i}.RDB{j}.conv{k}.0, model.1.sub.{n}, model.3 / 6 / 8
/ 10).  Anything else is refused by name.  The key tables are written from the public layouts; no real checkpoint has been loaded here.
"""
from __future__ import annotations

import re
from typing import Dict, Tuple

import torch

SCALE_OF_IN_CH = {3: 4, 12: 2, 48: 1}
_OLD_FIXED = {"model.0": "conv_first", "model.3": "conv_up1", "model.6": "conv_up2", "model.8": "conv_hr", "model.10": "conv_last"}
_OLD_RDB = re.compile(r"^model\.1\.sub\.(\d+)\.RDB([123])\.conv([1-5])\.0\.(weight|bias)$")
_OLD_BODY = re.compile(r"^model\.1\.sub\.(\d+)\.(weight|bias)$")


class UpscalerFormatError(ValueError):
    pass


def _looks_like(keys) -> str:
    ks = list(keys)
    has = lambda s: any(s in k for k in ks)
    if has("residual_group") or has("patch_embed"):
        return "a SwinIR / Swin2SR / HAT transformer"
    if has("attn.temperature") or has("adaptive") or has("before_RG"):
        return "a DAT transformer"
    if any(re.match(r"^body\.\d+\.(weight|bias)$", k) for k in ks):
        return "an SRVGGNetCompact (Real-ESRGAN 'compact') network"
    if has("model.1.sub."):
        return "an old-arch ESRGAN network at a scale other than 4 (its upsampling layers are not model.3 / model.6 / model.8 / model.10)"
    return "not an RRDBNet"


def normalize_state_dict(sd: Dict[str, torch.Tensor]) -> Tuple[Dict[str, torch.Tensor], str]:
    """-> (the state dict under BasicSR's "new" keys, "new" | "old"); raises UpscalerFormatError naming what the file looks like"""
    for wrap in ("params_ema", "params"):
        if wrap in sd and isinstance(sd[wrap], dict):
            sd = sd[wrap]
            break
    if "conv_first.weight" in sd and any(k.startswith("body.0.rdb1.") for k in sd):
        return dict(sd), "new"
    if "model.0.weight" in sd and any(_OLD_RDB.match(k) for k in sd):
        out, n_block = {}, 1 + max(int(m.group(1)) for m in map(_OLD_RDB.match, sd) if m)
        for k, v in sd.items():
            m = _OLD_RDB.match(k)
            if m:
                out[f"body.{m.group(1)}.rdb{m.group(2)}.conv{m.group(3)}.{m.group(4)}"] = v
                continue
            m = _OLD_BODY.match(k)
            if m and int(m.group(1)) == n_block:
                out[f"conv_body.{m.group(2)}"] = v
                continue
            base, _, leaf = k.rpartition(".")
            if base in _OLD_FIXED and leaf in ("weight", "bias"):
                out[f"{_OLD_FIXED[base]}.{leaf}"] = v
                continue
            raise UpscalerFormatError(f"upscaler: unexpected key {k!r} in an old-arch ESRGAN checkpoint: {_looks_like(sd)}; only the x4 "
                                      "layout (model.0, model.1.sub.*, model.3, model.6, model.8, model.10) is supported")
        return out, "old"
    raise UpscalerFormatError(f"upscaler: this checkpoint is {_looks_like(sd)}; only RRDBNet (ESRGAN, Real-ESRGAN x4plus / x2plus and "
                              "community models of that architecture) is supported")


def infer_geometry(sd: Dict[str, torch.Tensor]) -> dict:
    """sd under the "new" keys -> dict(num_block, nf, gc, in_ch, scale); every expected tensor is checked by name and shape, others refused"""
    w0 = sd["conv_first.weight"]
    nf, in_ch = int(w0.shape[0]), int(w0.shape[1])
    if in_ch not in SCALE_OF_IN_CH:
        raise UpscalerFormatError(f"upscaler: conv_first takes {in_ch} channels; RRDBNet takes 3 (x4), 12 (x2) or 48 (x1)")
    blocks = [int(k.split(".")[1]) for k in sd if k.startswith("body.")]
    num_block = 1 + max(blocks)
    gc = int(sd["body.0.rdb1.conv1.weight"].shape[0])
    want = {"conv_first": (nf, in_ch), "conv_body": (nf, nf), "conv_up1": (nf, nf), "conv_up2": (nf, nf), "conv_hr": (nf, nf), "conv_last": (3, nf)}
    for i in range(num_block):
        for j in (1, 2, 3):
            for k in (1, 2, 3, 4, 5):
                want[f"body.{i}.rdb{j}.conv{k}"] = (nf if k == 5 else gc, nf + (k - 1) * gc)
    for name, (co, ci) in want.items():
        w, b = sd.get(name + ".weight"), sd.get(name + ".bias")
        if w is None or b is None:
            raise UpscalerFormatError(f"upscaler: the checkpoint has no {name}.weight / .bias")
        if tuple(w.shape) != (co, ci, 3, 3) or tuple(b.shape) != (co,):
            raise UpscalerFormatError(f"upscaler: {name}.weight is {tuple(w.shape)}, expected {(co, ci, 3, 3)}")
    extra = sorted(set(sd) - {n + s for n in want for s in (".weight", ".bias")})
    if extra:
        raise UpscalerFormatError(f"upscaler: unexpected key {extra[0]!r} (+{len(extra) - 1} more): not a plain RRDBNet")
    if nf % 16 or gc % 16 or not (16 <= nf <= 64) or not (16 <= gc <= 64) or nf + 4 * gc > 256:
        raise UpscalerFormatError(f"upscaler: nf={nf}, gc={gc}: fluxmi_conv3x3_dense takes multiples of 16 with nf, gc <= 64 and nf + 4 gc <= 256")
    return dict(num_block=num_block, nf=nf, gc=gc, in_ch=in_ch, scale=SCALE_OF_IN_CH[in_ch])


def _pack(w: torch.Tensor, b: torch.Tensor, device):
    """Conv2d weight [Cout, Cin, 3, 3] / bias [Cout] -> the kernel's bf16 [Cout32, 3, 3, Cin16] / [Cout32], zero-padded"""
    co, ci = w.shape[0], w.shape[1]
    c32, c16 = -(-co // 32) * 32, -(-ci // 16) * 16
    w2 = torch.zeros(c32, 3, 3, c16, dtype=torch.bfloat16)
    w2[:co, :, :, :ci] = w.permute(0, 2, 3, 1).to(torch.bfloat16)
    b2 = torch.zeros(c32, dtype=torch.bfloat16)
    b2[:co] = b.to(torch.bfloat16)
    return w2.to(device), b2.to(device), co


class RRDBNet:
    """The network on one device; call it with NHWC bf16 RGB in [0, 1] -> NHWC bf16 at `scale` times the size.  upscale_uint8 wraps the value
    range: uint8 -> / 255 -> bf16 -> net -> clamp [0, 1] -> * 255, round half even -> uint8."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda:0"):
        sd, self.layout = normalize_state_dict(state_dict)
        g = infer_geometry(sd)
        self.num_block, self.nf, self.gc, self.in_ch, self.scale = g["num_block"], g["nf"], g["gc"], g["in_ch"], g["scale"]
        self.device = torch.device(device)
        names = {k.rsplit(".", 1)[0] for k in sd}
        self.layers = {n: _pack(sd[n + ".weight"], sd[n + ".bias"], self.device) for n in sorted(names)}

    # ---- limits ----------------------------------------------------------------------------------------------------------------------
    def memory_estimate(self, B: int, H: int, W: int) -> int:
        """bytes of activations the forward holds at its peak for a [B, H, W, 3] input: the larger of the trunk (four dense-block buffers,
        the head's features, the padded input) and the tail (conv_up2's and conv_hr's full-resolution outputs and the padded RGB)"""
        u = 4 // self.scale  # the net runs on the (H / u, W / u) grid
        px = B * (H // u) * (W // u)
        trunk = px * 2 * (4 * (self.nf + 4 * self.gc) + 2 * self.nf + 48)
        tail = px * 2 * (4 * self.nf + 16 * self.nf * 2 + 16 * 8)
        return max(trunk, tail)

    def check_input(self, B: int, H: int, W: int) -> None:
        """refuse, by name, what the kernel's addressing or the device's free memory cannot take"""
        from fluxmi import ops

        u = 4 // self.scale
        if B < 1 or H < 1 or W < 1 or H % u or W % u:
            raise ValueError(f"upscaler: a x{self.scale} RRDBNet needs B, H, W >= 1 and H, W multiples of {u} (pixel_unshuffle), got {B} x {H} x {W}")
        tiles = -(-(H // u * 4) // ops.CONV_DENSE_TILE)
        if B > 65535 or tiles > 65535:
            raise ValueError(f"upscaler: B={B} images / {tiles} tile rows exceed fluxmi_conv3x3_dense's launch grid (65535 each)")
        if self.device.type == "cuda":
            free = torch.cuda.mem_get_info(self.device)[0] + torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
            need = self.memory_estimate(B, H, W)
            if need > free:
                raise ValueError(f"upscaler: {B} x {H} x {W} needs about {need / 2 ** 30:.1f} GiB of activations, {free / 2 ** 30:.1f} GiB are "
                                 "free; the network is not tiled (its receptive field makes halo tiling inexact): send a smaller image")

    # ---- forward ---------------------------------------------------------------------------------------------------------------------
    def _conv(self, name, x, out, **kw):
        from fluxmi import ops

        w2, b2, _ = self.layers[name]
        return ops.conv3x3_dense(x, w2, b2, out, slope=0.2, **kw)

    @torch.inference_mode()
    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if x.ndim != 4 or x.shape[-1] != 3 or x.dtype != torch.bfloat16:
            raise ValueError(f"upscaler: expected NHWC bf16 RGB [B, H, W, 3], got {tuple(x.shape)} {x.dtype}")
        B, H0, W0, _ = x.shape
        self.check_input(B, H0, W0)
        x = x.to(self.device)
        u = 4 // self.scale
        if u > 1:  # Real-ESRGAN's pixel_unshuffle: channel (c, dy, dx) -> c * u * u + dy * u + dx
            x = x.view(B, H0 // u, u, W0 // u, u, 3).permute(0, 1, 3, 5, 2, 4).reshape(B, H0 // u, W0 // u, 3 * u * u)
        H, W = x.shape[1], x.shape[2]
        nf, gc, dev = self.nf, self.gc, self.device
        C = nf + 4 * gc
        new = lambda h, w, c: torch.empty(B, h, w, c, dtype=torch.bfloat16, device=dev)
        cin = self.layers["conv_first"][0].shape[-1]
        xin = torch.zeros(B, H, W, cin, dtype=torch.bfloat16, device=dev)
        xin[..., : self.in_ch] = x
        bufs = [new(H, W, C) for _ in range(4)]
        self._conv("conv_first", xin, bufs[0][..., :nf])
        feat = bufs[0][..., :nf].clone()
        cur = 0
        for i in range(self.num_block):
            ring = [bufs[(cur + j) % 4] for j in range(4)]
            for j in (1, 2, 3):
                src, dst = ring[j - 1], ring[j]
                for k in (1, 2, 3, 4):
                    lo = nf + (k - 1) * gc
                    self._conv(f"body.{i}.rdb{j}.conv{k}", src[..., :lo], src[..., lo : lo + gc], act=True)
                res2 = dict(r2=ring[0][..., :nf], a2=0.2) if j == 3 else {}
                self._conv(f"body.{i}.rdb{j}.conv5", src, dst[..., :nf], r1=src[..., :nf], a1=0.2, **res2)
            cur = (cur + 3) % 4
        t = new(H, W, nf)
        self._conv("conv_body", bufs[cur][..., :nf], t, r1=feat, a1=1.0)
        del bufs, ring, src, dst, feat, xin
        up1 = new(2 * H, 2 * W, nf)
        self._conv("conv_up1", t, up1, act=True, upsample=2)
        del t
        up2 = new(4 * H, 4 * W, nf)
        self._conv("conv_up2", up1, up2, act=True, upsample=2)
        del up1
        hr = new(4 * H, 4 * W, nf)
        self._conv("conv_hr", up2, hr, act=True)
        del up2
        rgb = new(4 * H, 4 * W, 8)[..., :3]
        self._conv("conv_last", hr, rgb)
        return rgb

    def upscale_uint8(self, px: torch.Tensor) -> torch.Tensor:
        """uint8 [B, H, W, 3] (any device) -> uint8 [B, scale H, scale W, 3] on the host"""
        if px.dtype != torch.uint8 or px.ndim != 4 or px.shape[-1] != 3:
            raise ValueError(f"upscaler: expected uint8 [B, H, W, 3], got {tuple(px.shape)} {px.dtype}")
        y = self(px.to(self.device).float().div(255.0).to(torch.bfloat16))
        return y.float().clamp(0.0, 1.0).mul(255.0).round().to(torch.uint8).cpu().contiguous()

    def upscale_uint8_device(self, px: torch.Tensor) -> torch.Tensor:
        """upscale_uint8's arithmetic with the result left on the network's device (contiguous): what the native JPEG encoder reads"""
        if px.dtype != torch.uint8 or px.ndim != 4 or px.shape[-1] != 3:
            raise ValueError(f"upscaler: expected uint8 [B, H, W, 3], got {tuple(px.shape)} {px.dtype}")
        y = self(px.to(self.device).float().div(255.0).to(torch.bfloat16))
        return y.float().clamp(0.0, 1.0).mul(255.0).round().to(torch.uint8).contiguous()


def read_upscaler(path: str, device="cuda:0") -> RRDBNet:
    """a LOCAL .safetensors or .pth (torch.load(weights_only=True)) file -> RRDBNet; nothing is downloaded"""
    if str(path).endswith(".safetensors"):
        from safetensors.torch import load_file

        sd = load_file(str(path), device="cpu")
    else:
        sd = torch.load(str(path), map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise UpscalerFormatError(f"upscaler: {path} does not hold a state dict")
    return RRDBNet(sd, device=device)
