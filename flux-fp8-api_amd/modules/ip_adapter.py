"""FLUX IP-Adapter (XLabs-AI `flux-ip-adapter` / `-v2` format) on MI355X: the image prompt enters every double block through its own small
cross-attention, with a strength the user sets.

What the adapter computes (XLabs' `IPDoubleStreamBlockProcessor` + `ImageProjModel`, RESTATED: neither XLabs' code nor diffusers is
available offline, so parity with them is unpinned -- DESIGN.md section 7; all arithmetic bf16, the linears plain nn.Linear, never quantised):
  1. image_embeds [n, 768] = CLIPVisionModelWithProjection(openai/clip-vit-large-patch14) of the CLIPImageProcessor-preprocessed image
     (`clip_preprocess`: RGB, bicubic resize of the short edge to 224, centre crop 224, x / 255, CLIP mean / std);
  2. projector `ip_adapter_proj_model`: proj = Linear(768, T * 4096) reshaped to [n, T, 4096], norm = LayerNorm(4096, eps 1e-5);
     T = proj.weight.shape[0] / 4096 (4 in v1);
  3. per double block i: k_ip = k_proj_i(tokens), v_ip = v_proj_i(tokens), each Linear(4096, hidden), keys
     `double_blocks.{i}.processor.ip_adapter_double_stream_{k,v}_proj.{weight,bias}`; no key norm, no RoPE.  Step-invariant: once per request;
  4. in the block: o = softmax(qn . k_ip^T * 128^-1/2) . v_ip with qn the block's image query after QK-RMSNorm and before RoPE, and
     img = img + ip_scale * o after the block's MLP residual (csrc/ip_attention.hip, one launch per double block inside the engine).
Several images concatenate their tokens (Nk = T * n <= 64): an extension of XLabs, as the image list is for Redux.

The projector and the 2 x depth linears run on libfluxmi's bf16 GEMM and `fluxmi_row_norm`; there is no PyTorch path.
"""
from __future__ import annotations

import re
from dataclasses import dataclass
from typing import Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor, nn

from modules.conditioner import _bf, _Cache, _lin

TOKEN_DIM = 4096   # the projector's token width (XLabs: cross_attention_dim)
CLIP_EMBED = 768   # CLIP ViT-L/14 projection_dim
MAX_TOKENS = 64    # fluxmi_ip_attention: 1 <= Nk <= 64
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
_BLOCK_KEY = re.compile(r"^double_blocks\.(\d+)\.processor\.ip_adapter_double_stream_(k|v)_proj\.(weight|bias)$")


@dataclass
class IPAdapterCall:
    """The `ip_adapter=` argument of Flux.forward / Flux.denoise: the step-invariant keys / values of every double block, bf16
    [depth, 1 or B, Nk, hidden] (a guided denoise call: [depth, 2 or 2B, ...], the prompt branches' first), and the strength: a float, `depth`
    floats (one per double block), or a [B, depth] tensor (per sample and block).  Never rounded to bf16."""
    k_ip: Tensor
    v_ip: Tensor
    scale: Union[float, Sequence[float], Tensor] = 1.0


def scale_table(scale, depth: int, batch: int) -> Tensor:
    """ip_adapter_scale -> float32 CPU tensor [batch, depth]: a float, `depth` floats, or a tensor [1 or batch, depth]"""
    if isinstance(scale, Tensor) and scale.ndim == 2:
        t = scale.detach().to(device="cpu", dtype=torch.float32)
        if t.shape[1] != depth or t.shape[0] not in (1, batch):
            raise ValueError(f"ip_adapter_scale: a table {tuple(t.shape)}, expected [1 or {batch}, {depth}]")
        t = t.expand(batch, depth)
    else:
        vals = [float(scale)] * depth if isinstance(scale, (int, float)) else [float(s) for s in scale]
        if len(vals) != depth:
            raise ValueError(f"ip_adapter_scale: {len(vals)} values for {depth} double blocks (a float, or one float per double block)")
        t = torch.tensor(vals, dtype=torch.float32)[None].expand(batch, depth)
    if not torch.isfinite(t).all():
        raise ValueError("ip_adapter_scale: not finite")
    return t.contiguous()


def clip_preprocess(image, size: int = 224) -> Tensor:
    """transformers' CLIPImageProcessor defaults -> fp32 [1, 3, size, size] on the host, bit for bit: RGB, PIL bicubic resize of the SHORT edge
    to `size` (the long edge int(size * long / short)), centre crop, x * (1 / 255) in float64 then float32, (x - mean) / std in float32."""
    from PIL import Image

    from modules.image_embedders import normalize_image, to_pil

    pil = to_pil(image).convert("RGB")
    w, h = pil.size
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    nw, nh = (new_short, new_long) if w <= h else (new_long, new_short)
    pil = pil.resize((nw, nh), resample=Image.BICUBIC)
    a = np.asarray(pil)
    top, left = (nh - size) // 2, (nw - size) // 2
    return normalize_image(a[top:top + size, left:left + size], CLIP_MEAN, CLIP_STD)


def check_state_dict(sd) -> tuple:
    """The loader's contract: the XLabs key names and shapes, anything else refused BY NAME -> (depth, T, hidden)."""
    keys = set(sd)
    if any(k.startswith(("image_proj.", "ip_adapter.")) for k in keys):
        raise ValueError("fluxmi: this is a diffusers-format IP-Adapter checkpoint (image_proj.* / ip_adapter.*); the loader takes the "
                         "XLabs format (ip_adapter_proj_model.*, double_blocks.{i}.processor.ip_adapter_double_stream_{k,v}_proj.*)")
    proj = ("ip_adapter_proj_model.proj.weight", "ip_adapter_proj_model.proj.bias", "ip_adapter_proj_model.norm.weight",
            "ip_adapter_proj_model.norm.bias")
    for k in proj:
        if k not in keys:
            raise ValueError(f"fluxmi: IP-Adapter checkpoint is missing {k}" + ("" if any(_BLOCK_KEY.match(x) for x in keys) else
                             " (not an XLabs flux-ip-adapter file: no ip_adapter_proj_model.* / double_blocks.*.processor.* keys)"))
    blocks = {}
    for k in keys:
        m = _BLOCK_KEY.match(k)
        if m:
            blocks.setdefault(int(m.group(1)), set()).add((m.group(2), m.group(3)))
        elif k not in proj:
            raise ValueError(f"fluxmi: IP-Adapter checkpoint has an unknown key {k}")
    if not blocks:
        raise ValueError("fluxmi: IP-Adapter checkpoint has no double_blocks.{i}.processor.ip_adapter_double_stream_{k,v}_proj.* keys")
    depth = max(blocks) + 1
    for i in range(depth):
        for kv in ("k", "v"):
            for wb in ("weight", "bias"):
                if (kv, wb) not in blocks.get(i, ()):
                    raise ValueError(f"fluxmi: IP-Adapter checkpoint is missing double_blocks.{i}.processor.ip_adapter_double_stream_{kv}_proj.{wb}")
    pw = sd["ip_adapter_proj_model.proj.weight"]
    if pw.ndim != 2 or pw.shape[1] != CLIP_EMBED or pw.shape[0] % TOKEN_DIM or pw.shape[0] == 0:
        raise ValueError(f"fluxmi: ip_adapter_proj_model.proj.weight {tuple(pw.shape)}: expected [T * {TOKEN_DIM}, {CLIP_EMBED}]")
    T = pw.shape[0] // TOKEN_DIM
    if T > MAX_TOKENS:
        raise ValueError(f"fluxmi: ip_adapter_proj_model.proj.weight gives {T} tokens per image, the adapter kernel takes at most {MAX_TOKENS}")
    for k, want in (("ip_adapter_proj_model.proj.bias", (T * TOKEN_DIM,)), ("ip_adapter_proj_model.norm.weight", (TOKEN_DIM,)),
                    ("ip_adapter_proj_model.norm.bias", (TOKEN_DIM,))):
        if tuple(sd[k].shape) != want:
            raise ValueError(f"fluxmi: {k} {tuple(sd[k].shape)}: expected {want}")
    w0 = sd["double_blocks.0.processor.ip_adapter_double_stream_k_proj.weight"]
    hidden = w0.shape[0] if w0.ndim == 2 else -1
    for i in range(depth):
        for kv in ("k", "v"):
            pre = f"double_blocks.{i}.processor.ip_adapter_double_stream_{kv}_proj."
            if tuple(sd[pre + "weight"].shape) != (hidden, TOKEN_DIM):
                raise ValueError(f"fluxmi: {pre}weight {tuple(sd[pre + 'weight'].shape)}: expected [{hidden}, {TOKEN_DIM}]")
            if tuple(sd[pre + "bias"].shape) != (hidden,):
                raise ValueError(f"fluxmi: {pre}bias {tuple(sd[pre + 'bias'].shape)}: expected [{hidden}]")
    return depth, T, hidden


class IPAdapter(nn.Module):
    """The projector and the 2 x depth key / value linears of an XLabs flux-ip-adapter checkpoint; `clip` is the vision tower
    (modules.image_embedders.ClipVisionNative, loaded from its own checkpoint) or None (image embeds are then given by the caller)."""

    def __init__(self, depth: int, num_tokens: int, hidden: int, clip=None):
        super().__init__()
        self.depth, self.num_tokens, self.hidden = int(depth), int(num_tokens), int(hidden)
        self.clip = clip
        self.ip_adapter_proj_model = nn.Module()
        self.ip_adapter_proj_model.proj = _lin(CLIP_EMBED, self.num_tokens * TOKEN_DIM, True)
        self.ip_adapter_proj_model.norm = nn.LayerNorm(TOKEN_DIM, eps=1e-5)
        self.k_proj = nn.ModuleList(_lin(TOKEN_DIM, hidden, True) for _ in range(depth))
        self.v_proj = nn.ModuleList(_lin(TOKEN_DIM, hidden, True) for _ in range(depth))
        self.requires_grad_(False)
        self._cache = _Cache()

    @classmethod
    def from_state_dict(cls, sd, clip=None) -> "IPAdapter":
        depth, T, hidden = check_state_dict(sd)
        m = cls(depth, T, hidden, clip)
        own = {}
        for k, v in sd.items():
            g = _BLOCK_KEY.match(k)
            own[f"{g.group(2)}_proj.{g.group(1)}.{g.group(3)}" if g else k] = v
        if clip is not None:
            own.update({"clip." + k: v for k, v in clip.state_dict().items()})
        nn.Module.load_state_dict(m, own, strict=True)
        return m

    @property
    def device(self):
        return self.ip_adapter_proj_model.proj.weight.device

    @torch.inference_mode()
    def tokens(self, image_embeds: Tensor) -> Tensor:
        """step 2: image_embeds [n, 768] -> bf16 [n * T, 4096], the images' tokens concatenated in list order"""
        from fluxmi import ops

        pm, ck = self.ip_adapter_proj_model, self._cache
        if image_embeds.ndim != 2 or image_embeds.shape[1] != CLIP_EMBED:
            raise ValueError(f"ip_adapter_image_embeds {tuple(image_embeds.shape)}: expected [n, {CLIP_EMBED}]")
        n = image_embeds.shape[0]
        if not 1 <= n * self.num_tokens <= MAX_TOKENS:
            raise ValueError(f"ip_adapter: {n} images x {self.num_tokens} tokens = {n * self.num_tokens} image tokens, the adapter takes 1..{MAX_TOKENS}")
        w, b, g, e = (ck.get(k, [t], lambda t=t: _bf(t)) for k, t in (("pw", pm.proj.weight), ("pb", pm.proj.bias), ("ng", pm.norm.weight),
                                                                        ("ne", pm.norm.bias)))
        x = image_embeds.to(device=self.device, dtype=torch.bfloat16).contiguous()
        t = ops.linear(x, w, b).view(n * self.num_tokens, TOKEN_DIM)
        return ops.row_norm(t, g, e, eps=1e-5, rms=False)

    @torch.inference_mode()
    def kv(self, image_embeds: Tensor):
        """step 3: image_embeds [n, 768] -> (k_ip, v_ip), each bf16 [depth, 1, n * T, hidden]"""
        from fluxmi import ops

        tok, ck = self.tokens(image_embeds), self._cache
        nk = tok.shape[0]
        k = torch.empty(self.depth, 1, nk, self.hidden, dtype=torch.bfloat16, device=tok.device)
        v = torch.empty_like(k)
        for i in range(self.depth):
            for out, lin, tag in ((k, self.k_proj[i], "k"), (v, self.v_proj[i], "v")):
                w, b = ck.get((tag + "w", i), [lin.weight], lambda lin=lin: _bf(lin.weight)), ck.get((tag + "b", i), [lin.bias], lambda lin=lin: _bf(lin.bias))
                ops.linear(tok, w, b, out=out[i, 0])
        return k, v

    @torch.inference_mode()
    def embed(self, images) -> Tensor:
        """step 1: one image or a list -> image_embeds bf16 [n, 768] through the CLIP vision tower"""
        if self.clip is None:
            raise RuntimeError("fluxmi: this IP-Adapter was loaded without a CLIP vision tower (clip_vision_path): pass ip_adapter_image_embeds")
        if not isinstance(images, (list, tuple)):
            images = [images]
        pix = torch.cat([clip_preprocess(im, self.clip.cfg["image_size"]) for im in images], 0).to(self.device)
        return self.clip(pix)["image_embeds"]

    def call(self, images=None, image_embeds: Optional[Tensor] = None, scale=1.0) -> IPAdapterCall:
        """the `ip_adapter=` argument for one branch: from images (through the tower) or from given embeds [n, 768]"""
        if (images is None) == (image_embeds is None):
            raise ValueError("ip_adapter: pass ip_adapter_image or ip_adapter_image_embeds, not both")
        k, v = self.kv(self.embed(images) if image_embeds is None else image_embeds)
        return IPAdapterCall(k, v, scale)


def read_ip_adapter(path: str, clip=None) -> IPAdapter:
    """one local .safetensors file in the XLabs format -> IPAdapter with its weights (host memory)"""
    from safetensors.torch import load_file

    return IPAdapter.from_state_dict(load_file(path, device="cpu"), clip)
