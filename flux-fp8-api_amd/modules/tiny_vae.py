"""The tiny autoencoder's decoder for FLUX latents (TAEF1: the 16-channel member of the TAESD family every FLUX front end ships for previews
and fast decodes) on the device: its residual blocks on the fused fluxmi_conv3x3_block (csrc/tiny_vae.hip), its other convolutions on
fluxmi_conv3x3_dense (csrc/upscaler.hip).  This docstring is the definition; no upstream file or code has been run against it (README).

  u    = z / scale_factor + shift_factor          z: the model's latent [B, 16, h, w], i.e. what AutoEncoder.decode takes; u: the
                                                  decoded-latent space the big decoder works in
  x    = relu(conv_1(3 tanh(u / 3)))              16 -> 64, bias
  x    = block_5(block_4(block_3(x)))             block(x) = relu(conv_c(relu(conv_b(relu(conv_a(x))))) + x), all 64 -> 64 with bias
  x    = block_10(block_9(block_8(conv_7(up2(x)))))       up2 = nearest 2x; conv_7, conv_12, conv_17: 64 -> 64 WITHOUT bias
  x    = block_15(block_14(block_13(conv_12(up2(x)))))
  x    = block_18(conv_17(up2(x)))
  y    = conv_19(x)                               64 -> 3, bias; RGB in [0, 1] at 8 h x 8 w
  out  = 2 y - 1                                  [B, 3, 8 h, 8 w] fp32 in the big decoder's range, so ONE uint8 rule serves both decoders:
                                                  FluxPipeline.to_uint8 (clamp to [-1, 1], (v + 1) * 127.5, truncate)

Every convolution is 3x3, stride 1, zero pad 1.  The subscripts are the indices of the original nn.Sequential (0 = the clamp, 2 = the stem's
ReLU, 6 / 11 / 16 = the upsamples).  Activations are NHWC bf16: the clamp is rounded to bf16 once, every launch rounds once, a block rounds
its two intermediates and its output (include/fluxmi.h).  The nearest upsamples are folded into conv_7 / 12 / 17 (upsample = 2).  Buffers are
allocated once per input shape and re-used.  17 launches: stem, 10 blocks, 3 upsampling convolutions, conv_19, and the two elementwise ends.

Checkpoints: a LOCAL .safetensors / .pth file with the original's bare Sequential keys ("1.weight", "3.conv.0.weight", .., "19.bias") or the
same behind "decoder." / "decoder.layers." (whose indices may start at the stem: the offset is taken from where the [64, 16, 3, 3] weight
sits).  "encoder." keys are ignored; any other key or shape is refused by name.  The encoder is out of scope.
"""
from __future__ import annotations

import re
from typing import Dict

import torch

_KEY = re.compile(r"^(decoder\.layers\.|decoder\.|)(\d+)\.(?:conv\.([024])\.)?(weight|bias)$")
BLOCKS = (3, 4, 5, 8, 9, 10, 13, 14, 15, 18)  # Sequential indices of the residual blocks
UPCONVS = (7, 12, 17)                          # ... of the bias-free convolutions behind the upsamples
STEM, LAST = 1, 19


class TinyAEFormatError(ValueError):
    pass


def normalize_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """-> the decoder's tensors under the bare Sequential keys with the stem at index 1; refuses anything that is not this decoder"""
    found = {}
    for k, v in sd.items():
        if k.startswith("encoder."):
            continue
        m = _KEY.match(k)
        if not m or not isinstance(v, torch.Tensor):
            raise TinyAEFormatError(f"tiny_vae: unexpected key {k!r}: not a TAEF1 decoder (bare Sequential keys, or behind decoder. / decoder.layers.)")
        found[(m.group(1), int(m.group(2)), m.group(3), m.group(4))] = v
    stems = [key for key, v in found.items() if key[2] is None and key[3] == "weight" and tuple(v.shape) == (64, 16, 3, 3)]
    if len(stems) != 1 or len({key[0] for key in found}) != 1:
        raise TinyAEFormatError("tiny_vae: the file has no single [64, 16, 3, 3] stem convolution under one key prefix: not a TAEF1 decoder "
                                "(TAESD for 4-channel latents and other widths are not covered)")
    off = stems[0][1] - STEM
    out = {}
    for (_, idx, sub, leaf), v in found.items():
        out[f"{idx - off}." + (f"conv.{sub}." if sub is not None else "") + leaf] = v
    want = {f"{STEM}.weight": (64, 16, 3, 3), f"{STEM}.bias": (64,), f"{LAST}.weight": (3, 64, 3, 3), f"{LAST}.bias": (3,)}
    want.update({f"{i}.weight": (64, 64, 3, 3) for i in UPCONVS})
    for i in BLOCKS:
        for s in (0, 2, 4):
            want[f"{i}.conv.{s}.weight"], want[f"{i}.conv.{s}.bias"] = (64, 64, 3, 3), (64,)
    for name, shape in want.items():
        if name not in out or tuple(out[name].shape) != shape:
            got = tuple(out[name].shape) if name in out else "missing"
            raise TinyAEFormatError(f"tiny_vae: layer {name} is {got}, expected {shape}: not the 64-channel TAEF1 decoder")
    extra = sorted(set(out) - set(want))
    if extra:
        raise TinyAEFormatError(f"tiny_vae: unexpected tensor {extra[0]!r} (+{len(extra) - 1} more): not the TAEF1 decoder")
    return out


def _nhwc(w: torch.Tensor) -> torch.Tensor:
    return w.permute(0, 2, 3, 1).to(torch.bfloat16).contiguous()  # Conv2d [Cout, Cin, 3, 3] -> the kernels' [Cout, 3, 3, Cin]


class TinyDecoder:
    """The decoder on one device.  decode(z): the model's latent [B, 16, h, w] -> [B, 3, 8 h, 8 w] fp32 in [-1, 1] (unclamped), where
    AutoEncoder.decode would put it."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda:0", scale_factor: float = 1.0, shift_factor: float = 0.0):
        sd = normalize_state_dict(state_dict)
        self.device = torch.device(device)
        self.scale_factor, self.shift_factor = float(scale_factor), float(shift_factor)
        dev = self.device
        self.stem = (_nhwc(sd[f"{STEM}.weight"]).to(dev), sd[f"{STEM}.bias"].to(torch.bfloat16).to(dev))
        self.blocks = {i: (torch.stack([_nhwc(sd[f"{i}.conv.{s}.weight"]) for s in (0, 2, 4)]).to(dev),
                           torch.stack([sd[f"{i}.conv.{s}.bias"].to(torch.bfloat16) for s in (0, 2, 4)]).to(dev)) for i in BLOCKS}
        self.upconvs = {i: _nhwc(sd[f"{i}.weight"]).to(dev) for i in UPCONVS}
        w_last = torch.zeros(32, 3, 3, 64, dtype=torch.bfloat16)
        w_last[:3] = _nhwc(sd[f"{LAST}.weight"])
        b_last = torch.zeros(32, dtype=torch.bfloat16)
        b_last[:3] = sd[f"{LAST}.bias"].to(torch.bfloat16)
        self.last = (w_last.to(dev), b_last.to(dev))
        self._bufs = {}

    def check_input(self, B: int, h: int, w: int) -> None:
        from fluxmi import ops

        if B < 1 or h < 1 or w < 1 or B > 65535 or -(-8 * h // ops.CONV_DENSE_TILE) > 65535:
            raise ValueError(f"tiny_vae: a latent batch of {B} x {h} x {w} is outside the convolution kernels' launch grid (1..65535 images and tile rows)")

    def _buffers(self, B: int, h: int, w: int):
        key = (B, h, w)
        if key not in self._bufs:
            new = lambda H, W, C: torch.empty(B, H, W, C, dtype=torch.bfloat16, device=self.device)
            self._bufs = {key: dict(xin=new(h, w, 16), rgb=new(8 * h, 8 * w, 8),
                                    lvl=[(new(h << s, w << s, 64), new(h << s, w << s, 64)) for s in range(4)])}  # one shape is kept
        return self._bufs[key]

    def _block(self, i: int, x: torch.Tensor, out: torch.Tensor) -> None:
        from fluxmi import ops

        ops.conv3x3_block(x, self.blocks[i][0], self.blocks[i][1], out)

    @torch.inference_mode()
    def decode_nhwc(self, z: torch.Tensor) -> torch.Tensor:
        """-> y, the network's RGB in [0, 1]: a bf16 [B, 8 h, 8 w, 3] window of a buffer the next call overwrites"""
        from fluxmi import ops

        if z.ndim != 4 or z.shape[1] != 16:
            raise ValueError(f"tiny_vae: expected a latent [B, 16, h, w], got {tuple(z.shape)}")
        B, _, h, w = z.shape
        self.check_input(B, h, w)
        buf = self._buffers(B, h, w)
        with torch.cuda.device(self.device):  # the kernels launch on the current stream of the current device
            u = z.to(self.device).float() / self.scale_factor + self.shift_factor
            buf["xin"].copy_((3.0 * torch.tanh(u / 3.0)).permute(0, 2, 3, 1))
            a, b = buf["lvl"][0]
            ops.conv3x3_dense(buf["xin"], self.stem[0], self.stem[1], a, slope=0.0, act=True)
            order = iter(BLOCKS)
            for lvl, n_blocks in enumerate((3, 3, 3, 1)):
                if lvl:
                    src, (a, b) = a, buf["lvl"][lvl]
                    ops.conv3x3_dense(src, self.upconvs[UPCONVS[lvl - 1]], None, a, upsample=2)
                for _ in range(n_blocks):
                    self._block(next(order), a, b)
                    a, b = b, a
            rgb = buf["rgb"][..., :3]
            ops.conv3x3_dense(a, self.last[0], self.last[1], rgb)
        return rgb

    def decode(self, z: torch.Tensor) -> torch.Tensor:
        return self.decode_nhwc(z).permute(0, 3, 1, 2).float().mul(2.0).sub(1.0)


def read_tiny_ae(path: str, device="cuda:0", scale_factor: float = 1.0, shift_factor: float = 0.0) -> TinyDecoder:
    """a LOCAL .safetensors or .pth (torch.load(weights_only=True)) file -> TinyDecoder; nothing is downloaded"""
    if str(path).endswith(".safetensors"):
        from safetensors.torch import load_file

        sd = load_file(str(path), device="cpu")
    else:
        sd = torch.load(str(path), map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise TinyAEFormatError(f"tiny_vae: {path} does not hold a state dict")
    return TinyDecoder(sd, device=device, scale_factor=scale_factor, shift_factor=shift_factor)
