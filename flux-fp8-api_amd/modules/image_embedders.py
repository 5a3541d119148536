"""Image conditioning on MI355X -- FLUX.1 Redux [dev]: BFL's `ReduxImageEncoder` (src/flux/modules/image_embedders.py) over a native SigLIP.

What Redux computes (BFL `ReduxImageEncoder.__call__` + `prepare_redux`, src/flux/sampling.py), kept here in one place:
  1. preprocessing = transformers' SiglipImageProcessor of google/siglip-so400m-patch14-384: convert to RGB, PIL bicubic resize to
     384 x 384, x / 255 (in float64, then float32), normalise with mean = std = 0.5 -> pixel_values fp32 [1, 3, 384, 384], cast to bf16;
  2. SiglipVisionModel(...).last_hidden_state in bf16: a stride-14 "valid" Conv2d(3, 1152, 14) (a 27 x 27 grid = 729 tokens; the last 6
     pixel rows and columns are never read) + position embedding [729, 1152]; 27 pre-LN encoder layers (LayerNorm eps 1e-6 with bias;
     q/k/v/out projections with bias, 16 heads of 72, non-causal, scale 72^-1/2; LayerNorm; fc1 1152 -> 4304, gelu_pytorch_tanh, fc2
     4304 -> 1152; both residual adds in bf16); post_layernorm.  The pooling head (vision_model.head.*) is not used;
  3. projector: redux_down(silu(redux_up(x))), Linear(1152, 12288) and Linear(12288, 4096) with bias, bf16 -> [1, 729, 4096] bf16;
  4. txt = cat(t5_embedding, redux_tokens, dim=-2), repeated over the batch; txt_ids = zeros(bs, Lt, 3); vec (CLIP) unchanged.  The flow
     model is plain Flux-dev / Flux-schnell; schedule, noise draw and guidance do not change (FluxPipeline.prepare_redux_tokens).

The encoder runs on libfluxmi: every Linear on the bf16 MFMA GEMM (residual adds and the position embedding in its gate*y+x epilogue
with a ones gate), LayerNorm = `fluxmi_row_norm`, gelu_tanh / silu = `fluxmi_act`, attention = `fluxmi_vision_attention` (all images of a
call in one launch), the patch embedding = `fluxmi_patchify_rect` + the GEMM; modules/encoder_common.py has the layer, shared with the
other towers.  So that every GEMM takes a tiled config, weights are padded once at load time (exact: the pads are zeros):
  * heads of 72 -> 96: q / k / v weight rows and biases per head, out_proj's columns per head.  Zero q / k columns add nothing to q.k,
    zero V^T rows and v_bias entries give zero output columns, and out_proj's zero columns drop them;
  * fc1 rows / bias and fc2 columns to a multiple of 256 (4304 -> 4352): gelu_tanh(0) = 0;
  * the patch matrix's K from 3 * 14 * 14 = 588 to 640 (1280 bytes per row).
q | k run as one GEMM; V^T comes from the v-projection GEMM with its operands swapped (the text encoders' scheme), its bias added after
P V (rows of P sum to 1).  A sequence is padded to Lp = 768 rows (729 -> a multiple of 256: the GEMM tiles' and V^T's column count).
"""
from __future__ import annotations

import io
import json
import os
from typing import Optional

import numpy as np
import torch
from torch import Tensor, nn

from modules.conditioner import _read_dir_weights
from modules.encoder_common import (CLIP_LAYER, _bf, _Cache, _lin, _linear_groups, _pad_to, _round_up, _Weight,  # noqa: F401  (re-exported)
                                    clip_encoder_layers, encoder_layer, layer_weights, normalize_image, pad_heads, padded_head_dim, patch_embed,
                                    unpad_heads, vision_attend)

# google/siglip-so400m-patch14-384 (the vision tower FLUX.1 Redux was trained on); keys left out of a config mean SiglipVisionConfig's
# defaults, as transformers reads them
SIGLIP_SO400M_384 = dict(hidden_size=1152, intermediate_size=4304, num_hidden_layers=27, num_attention_heads=16, num_channels=3,
                         image_size=384, patch_size=14, hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-6)
_SIGLIP_DEFAULTS = dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, num_channels=3,
                        image_size=224, patch_size=16, hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-6)


# ---- SigLIP vision tower ------------------------------------------------------------------------------------------------------------
class _SiglipVisionTransformer(nn.Module):
    def __init__(self, c):
        super().__init__()
        D, Fd, C, P = c["hidden_size"], c["intermediate_size"], c["num_channels"], c["patch_size"]
        self.embeddings = nn.Module()
        self.embeddings.patch_embedding = nn.Conv2d(C, D, kernel_size=P, stride=P)
        self.embeddings.position_embedding = _Weight((c["image_size"] // P) ** 2, D)
        self.encoder = nn.Module()
        self.encoder.layers = clip_encoder_layers(c["num_hidden_layers"], D, Fd, c["layer_norm_eps"])
        self.post_layernorm = nn.LayerNorm(D, eps=c["layer_norm_eps"])
        self.requires_grad_(False)


class SiglipVisionNative(nn.Module):
    """State-dict keys of transformers' SiglipVisionModel: vision_model.embeddings.{patch_embedding, position_embedding},
    vision_model.encoder.layers.{i}.{self_attn.{q,k,v,out}_proj, layer_norm1, layer_norm2, mlp.fc1, mlp.fc2}, vision_model.post_layernorm.
    A full SiglipModel checkpoint loads too: text_model.*, logit_scale, logit_bias and the pooling head vision_model.head.* are ignored.
    `config`: a SiglipVisionConfig dict, or a SiglipModel config.json (its `vision_config`); None = google/siglip-so400m-patch14-384."""

    def __init__(self, config: Optional[dict] = None):
        super().__init__()
        c = dict(_SIGLIP_DEFAULTS)
        if config is None:
            c.update(SIGLIP_SO400M_384)
        elif "vision_config" in config:
            c.update(config.get("vision_config") or {})
        else:
            c.update(config)
        if c["hidden_act"] not in ("gelu_pytorch_tanh", "gelu_new"):
            raise ValueError(f"fluxmi: the native SigLIP covers gelu_pytorch_tanh MLPs, got {c['hidden_act']!r}")
        D, H = c["hidden_size"], c["num_attention_heads"]
        if D % H or D % 8:
            raise ValueError(f"fluxmi: hidden_size {D} must be a multiple of the head count {H} and of 8")
        self.cfg = c
        self.head_dim = D // H
        self.head_pad = padded_head_dim(self.head_dim)
        self.grid = c["image_size"] // c["patch_size"]
        self.num_tokens = self.grid ** 2
        self.vision_model = _SiglipVisionTransformer(c)
        self._cache = _Cache()

    def load_state_dict(self, sd, strict=True, assign=False):
        sd = {k: v for k, v in sd.items() if not k.startswith(("text_model.", "logit_scale", "logit_bias")) and not k.endswith("position_ids")}
        # keys without the `vision_model.` prefix (how transformers 5.x saves a bare SiglipVisionModel) are accepted too
        sd = {(k if k.startswith("vision_model.") else "vision_model." + k): v for k, v in sd.items()}
        return super().load_state_dict({k: v for k, v in sd.items() if not k.startswith("vision_model.head.")}, strict=strict, assign=assign)

    @property
    def device(self):
        return self.vision_model.post_layernorm.weight.device

    @property
    def seq_pad(self) -> int:
        """rows a sequence is padded to: a multiple of 256 (the GEMM tile height; also V^T's column count, which the swapped v-projection
        GEMM needs as a multiple of its 256-column tile)"""
        return _round_up(self.num_tokens, 256)

    @property
    def mlp_pad(self) -> int:
        return _round_up(self.cfg["intermediate_size"], 256)

    @property
    def patch_k(self) -> int:
        c = self.cfg
        return _round_up(c["num_channels"] * c["patch_size"] ** 2, 64)

    def padded_weights(self, i) -> dict:
        """bf16 weights of layer i (or i = "embed") as the kernels take them, built once (see the module docstring for the padding)"""
        vm, ck, c = self.vision_model, self._cache, self.cfg
        if i == "embed":
            pe = vm.embeddings.patch_embedding
            return dict(
                w=ck.get("patch_w", [pe.weight], lambda: _pad_to(_bf(pe.weight).reshape(pe.weight.shape[0], -1), self.patch_k, 1).contiguous()),
                b=ck.get("patch_b", [pe.bias], lambda: _bf(pe.bias)),
                pos=ck.get("pos", [vm.embeddings.position_embedding.weight], lambda: _bf(vm.embeddings.position_embedding.weight)))
        return layer_weights(ck, vm.encoder.layers[i], CLIP_LAYER, i, c["num_attention_heads"], self.head_dim, self.head_pad, self.mlp_pad)

    @torch.inference_mode()
    def forward(self, pixel_values: Tensor, **_) -> dict:
        """pixel_values [B, C, image_size, image_size] -> {"last_hidden_state": bf16 [B, grid^2, hidden]}"""
        from fluxmi import ops

        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("fluxmi: the SigLIP vision encoder needs the GPU (libfluxmi has no CPU path)")
        c, ck, vm = self.cfg, self._cache, self.vision_model
        D, H, eps, P, S = c["hidden_size"], c["num_attention_heads"], c["layer_norm_eps"], c["patch_size"], c["image_size"]
        pix = pixel_values.to(device=dev, dtype=torch.bfloat16)
        if pix.dim() != 4 or pix.shape[1] != c["num_channels"] or tuple(pix.shape[-2:]) != (S, S):
            raise ValueError(f"fluxmi: SigLIP takes pixel_values [B, {c['num_channels']}, {S}, {S}], got {tuple(pix.shape)}")
        B, L, Lp, hp = pix.shape[0], self.num_tokens, self.seq_pad, self.head_pad
        ones = ck.get("ones", [vm.post_layernorm.weight], lambda: torch.ones(D, dtype=torch.bfloat16, device=dev))
        # patch embedding + position embedding: bf16(pos + bf16(conv)), written into the first L rows of each image's Lp-row slab
        e = self.padded_weights("embed")
        x = patch_embed(pix, P, self.grid, self.grid, self.patch_k, e["w"], e["b"], e["pos"], None, Lp, ones)
        attend, gelu_tanh = vision_attend(B, L, Lp, H, self.head_dim, hp), lambda f: ops.act(f, 0)  # noqa: E731
        for i in range(len(vm.encoder.layers)):
            x = encoder_layer(x, self.padded_weights(i), attend, gelu_tanh, eps, ones, ones)
        g, e2 = (ck.get((n, "post"), [t], lambda t=t: _bf(t)) for n, t in (("g", vm.post_layernorm.weight), ("e", vm.post_layernorm.bias)))
        y = ops.row_norm(x, g, e2, eps=eps, rms=False).view(B, Lp, D)[:, :L]
        return {"last_hidden_state": y.contiguous()}


# ---- FLUX.1 Redux ------------------------------------------------------------------------------------------------------------------
def to_pil(image):
    """str (path, or base64 / data-URL) | PIL.Image | np.ndarray (uint8 HW / HWC) | torch.Tensor (uint8 HW / HWC) -> PIL.Image"""
    from base64 import standard_b64decode

    from PIL import Image

    if isinstance(image, Image.Image):
        return image
    if isinstance(image, str):
        try:
            return Image.open(image)
        except Exception:
            return Image.open(io.BytesIO(standard_b64decode(image.split(",")[-1])))
    if isinstance(image, torch.Tensor):
        image = image.detach().cpu()
        if image.dtype != torch.uint8:
            raise TypeError(f"fluxmi: an image tensor must be uint8 HW / HWC, got {image.dtype}")
        image = image.numpy()
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8:
            raise TypeError(f"fluxmi: an image array must be uint8 HW / HWC, got {image.dtype}")
        return Image.fromarray(image)
    raise TypeError(f"fluxmi: cannot read an image from {type(image).__name__}")


class ReduxImageEncoder(nn.Module):
    """BFL's ReduxImageEncoder (src/flux/modules/image_embedders.py): keys redux_up.{weight,bias} / redux_down.{weight,bias} of
    flux1-redux-dev.safetensors; `siglip` is the vision tower (SiglipVisionNative, loaded from its own checkpoint)."""

    def __init__(self, siglip: SiglipVisionNative, txt_in_features: int = 4096):
        super().__init__()
        d = siglip.cfg["hidden_size"]
        self.siglip = siglip
        self.redux_up = _lin(d, 3 * txt_in_features, True)
        self.redux_down = _lin(3 * txt_in_features, txt_in_features, True)
        self.image_size = siglip.cfg["image_size"]
        self._cache = _Cache()

    def load_state_dict(self, sd, strict=True, assign=False):
        """the projector's own keys (a Redux checkpoint); the SigLIP tower loads through self.siglip"""
        sd = {k: v for k, v in sd.items() if k.startswith(("redux_up.", "redux_down."))}
        missing = [k for k in ("redux_up.weight", "redux_up.bias", "redux_down.weight", "redux_down.bias") if k not in sd]
        if missing and strict:
            raise RuntimeError(f"fluxmi: Redux checkpoint is missing {missing}")
        self.redux_up.load_state_dict({k[len("redux_up."):]: v for k, v in sd.items() if k.startswith("redux_up.")}, strict=strict, assign=assign)
        self.redux_down.load_state_dict({k[len("redux_down."):]: v for k, v in sd.items() if k.startswith("redux_down.")}, strict=strict,
                                        assign=assign)
        return nn.modules.module._IncompatibleKeys(missing, [])

    @property
    def device(self):
        return self.redux_up.weight.device

    @property
    def num_tokens(self) -> int:
        return self.siglip.num_tokens

    def preprocess(self, image) -> Tensor:
        """step 1 of the module docstring -> fp32 [1, 3, S, S] on the host (S = 384), bit-identical to transformers'
        SiglipImageProcessor(size={"height": S, "width": S}).  `image`: anything to_pil takes."""
        from PIL import Image

        pil = to_pil(image).convert("RGB").resize((self.image_size, self.image_size), resample=Image.BICUBIC)
        return normalize_image(np.asarray(pil), np.float32(0.5), np.float32(0.5))

    @torch.inference_mode()
    def project(self, hidden: Tensor) -> Tensor:
        """step 3: [n, T, 1152] bf16 -> redux_down(silu(redux_up(x))) [n, T, 4096] bf16"""
        from fluxmi import ops

        n, T, d = hidden.shape
        ck = self._cache
        wu, bu, wd, bd = (ck.get(k, [t], lambda t=t: _bf(t)) for k, t in (("wu", self.redux_up.weight), ("bu", self.redux_up.bias),
                                                                            ("wd", self.redux_down.weight), ("bd", self.redux_down.bias)))
        up = ops.act(ops.linear(hidden.reshape(n * T, d).contiguous(), wu, bu), 1)
        return ops.linear(up, wd, bd).view(n, T, -1)

    @torch.inference_mode()
    def __call__(self, images) -> Tensor:
        """one image or a list -> Redux tokens bf16 [n, 729, 4096] on the encoder's device, in list order"""
        if not isinstance(images, (list, tuple)):
            images = [images]
        pix = torch.cat([self.preprocess(im) for im in images], 0).to(self.device)
        return self.project(self.siglip(pix)["last_hidden_state"])


def _read_tower(path: str, cls, what: str):
    """a local HF directory (config.json + *.safetensors) or one .safetensors file (cls's default geometry) -> cls with its weights (host memory)"""
    from safetensors.torch import load_file

    cfg = None
    if os.path.isdir(path):
        cj = os.path.join(path, "config.json")
        if os.path.exists(cj):
            with open(cj) as f:
                cfg = json.load(f)
        sd = _read_dir_weights(path)
    else:
        sd = load_file(path, device="cpu")
    m = cls(cfg)
    missing, _ = m.load_state_dict(sd, strict=False)
    if missing:
        raise RuntimeError(f"fluxmi: {what} checkpoint is missing weights: {missing[:4]} ...")
    return m


def read_siglip(path: str) -> SiglipVisionNative:
    """a local HF directory (config.json + *.safetensors of SiglipVisionModel or SiglipModel) or one .safetensors file (the
    so400m-patch14-384 geometry) -> SiglipVisionNative with its weights (host memory)"""
    return _read_tower(path, SiglipVisionNative, "SigLIP")


# ---- CLIP vision tower (the IP-Adapter's image encoder; modules/ip_adapter.py) -----------------------------------------------------------
# openai/clip-vit-large-patch14's vision_config; keys left out of a config mean CLIPVisionConfig's defaults, as transformers reads them
CLIP_VIT_L14 = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, num_channels=3, image_size=224,
                    patch_size=14, hidden_act="quick_gelu", layer_norm_eps=1e-5, projection_dim=768)
_CLIP_VISION_DEFAULTS = dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, num_channels=3,
                             image_size=224, patch_size=32, hidden_act="quick_gelu", layer_norm_eps=1e-5, projection_dim=512)


class _ClipVisionTransformer(nn.Module):
    def __init__(self, c):
        super().__init__()
        D, Fd, C, P = c["hidden_size"], c["intermediate_size"], c["num_channels"], c["patch_size"]
        self.embeddings = nn.Module()
        self.embeddings.class_embedding = nn.Parameter(torch.zeros(D))
        self.embeddings.patch_embedding = nn.Conv2d(C, D, kernel_size=P, stride=P, bias=False)
        self.embeddings.position_embedding = _Weight((c["image_size"] // P) ** 2 + 1, D)
        self.pre_layrnorm = nn.LayerNorm(D, eps=c["layer_norm_eps"])  # (transformers' spelling: it is the state-dict key)
        self.encoder = nn.Module()
        self.encoder.layers = clip_encoder_layers(c["num_hidden_layers"], D, Fd, c["layer_norm_eps"])
        self.post_layernorm = nn.LayerNorm(D, eps=c["layer_norm_eps"])
        self.requires_grad_(False)


class ClipVisionNative(nn.Module):
    """transformers' CLIPVisionModelWithProjection on libfluxmi, built from the kernels the SigLIP tower runs on (no kernel of its own):
    class token + stride-P "valid" Conv2d without bias (fluxmi_patchify_rect + GEMM) + position embedding; pre_layrnorm; pre-LN encoder layers
    (LayerNorm eps 1e-5 with bias; q / k / v / out projections with bias, heads of 64, non-causal, scale 64^-1/2 through
    fluxmi_vision_attention; fc1, quick_gelu = `ops.act_mul(x, gated=False)`, fc2; both residual adds in bf16); post_layernorm on the class
    token; visual_projection without bias -> image_embeds.  State-dict keys: vision_model.embeddings.{class_embedding, patch_embedding,
    position_embedding}, vision_model.pre_layrnorm, vision_model.encoder.layers.{i}.*, vision_model.post_layernorm, visual_projection.  A
    full CLIPModel checkpoint loads too: text_model.*, text_projection and logit_scale are ignored.
    A sequence of grid^2 + 1 tokens (257 for ViT-L/14) is padded to a multiple of 256 rows (512), fc1 / fc2 to a multiple of 256 and the
    patch matrix's K to a multiple of 64, as for SigLIP (zeros: exact).
    `config`: a CLIPVisionConfig dict or a CLIPModel config.json (its `vision_config` + `projection_dim`); None = openai/clip-vit-large-patch14."""

    def __init__(self, config: Optional[dict] = None):
        super().__init__()
        c = dict(_CLIP_VISION_DEFAULTS)
        if config is None:
            c.update(CLIP_VIT_L14)
        elif "vision_config" in config:
            c.update(config.get("vision_config") or {})
            if "projection_dim" in config:
                c["projection_dim"] = config["projection_dim"]
        else:
            c.update(config)
        if c["hidden_act"] != "quick_gelu":
            raise ValueError(f"fluxmi: the native CLIP vision tower covers quick_gelu MLPs, got {c['hidden_act']!r}")
        D, H = c["hidden_size"], c["num_attention_heads"]
        if D % H or D % 8 or D // H > 64:
            raise ValueError(f"fluxmi: CLIP vision hidden_size {D} must be a multiple of 8 and of the head count {H}, with heads of at most 64")
        self.cfg = c
        self.head_dim = D // H
        self.head_pad = padded_head_dim(self.head_dim)
        self.grid = c["image_size"] // c["patch_size"]
        self.num_tokens = self.grid ** 2 + 1
        self.vision_model = _ClipVisionTransformer(c)
        self.visual_projection = _lin(D, c["projection_dim"], False)
        self._cache = _Cache()

    def load_state_dict(self, sd, strict=True, assign=False):
        sd = {k: v for k, v in sd.items() if not k.startswith(("text_model.", "text_projection", "logit_scale")) and not k.endswith("position_ids")}
        return super().load_state_dict(sd, strict=strict, assign=assign)

    @property
    def device(self):
        return self.vision_model.post_layernorm.weight.device

    @property
    def seq_pad(self) -> int:
        return _round_up(self.num_tokens, 256)

    @property
    def mlp_pad(self) -> int:
        return _round_up(self.cfg["intermediate_size"], 256)

    @property
    def patch_k(self) -> int:
        c = self.cfg
        return _round_up(c["num_channels"] * c["patch_size"] ** 2, 64)

    def padded_weights(self, i) -> dict:
        """bf16 weights of layer i (or i = "embed") as the kernels take them, built once"""
        vm, ck, c = self.vision_model, self._cache, self.cfg
        if i == "embed":
            em = vm.embeddings
            pe, pos = em.patch_embedding, em.position_embedding.weight
            return dict(
                w=ck.get("patch_w", [pe.weight], lambda: _pad_to(_bf(pe.weight).reshape(pe.weight.shape[0], -1), self.patch_k, 1).contiguous()),
                pos=ck.get("pos", [pos], lambda: _bf(pos)),
                # the class row: bf16(class_embedding + position_embedding[0]) on bf16 tensors, as transformers adds them
                cls=ck.get("cls", [em.class_embedding, pos], lambda: (_bf(em.class_embedding) + _bf(pos)[0]).contiguous()))
        return layer_weights(ck, vm.encoder.layers[i], CLIP_LAYER, i, c["num_attention_heads"], self.head_dim, self.head_pad, self.mlp_pad)

    @torch.inference_mode()
    def forward(self, pixel_values: Tensor, **_) -> dict:
        """pixel_values [B, C, image_size, image_size] -> {"image_embeds": bf16 [B, projection_dim], "last_hidden_state": bf16
        [B, grid^2 + 1, hidden] (before post_layernorm, as transformers returns it)}"""
        from fluxmi import ops

        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("fluxmi: the CLIP vision encoder needs the GPU (libfluxmi has no CPU path)")
        c, ck, vm = self.cfg, self._cache, self.vision_model
        D, H, eps, P, S = c["hidden_size"], c["num_attention_heads"], c["layer_norm_eps"], c["patch_size"], c["image_size"]
        pix = pixel_values.to(device=dev, dtype=torch.bfloat16)
        if pix.dim() != 4 or pix.shape[1] != c["num_channels"] or tuple(pix.shape[-2:]) != (S, S):
            raise ValueError(f"fluxmi: CLIP takes pixel_values [B, {c['num_channels']}, {S}, {S}], got {tuple(pix.shape)}")
        B, L, Lp, hp = pix.shape[0], self.num_tokens, self.seq_pad, self.head_pad
        ones = ck.get("ones", [vm.post_layernorm.weight], lambda: torch.ones(D, dtype=torch.bfloat16, device=dev))
        ln = lambda x, mod, tag: ops.row_norm(x, ck.get((tag, "g"), [mod.weight], lambda: _bf(mod.weight)),  # noqa: E731
                                              ck.get((tag, "e"), [mod.bias], lambda: _bf(mod.bias)), eps=eps, rms=False)
        # row 0 of each image's Lp-row slab: the class row; rows 1 .. G: bf16(pos + bf16(conv)); the rest zero (finite through every layer)
        e = self.padded_weights("embed")
        x = ln(patch_embed(pix, P, self.grid, self.grid, self.patch_k, e["w"], None, e["pos"][1:], e["cls"], Lp, ones), vm.pre_layrnorm, "pre")
        attend, quick_gelu = vision_attend(B, L, Lp, H, self.head_dim, hp), lambda f: ops.act_mul(f, gated=False)  # noqa: E731
        for i in range(len(vm.encoder.layers)):
            x = encoder_layer(x, self.padded_weights(i), attend, quick_gelu, eps, ones, ones)
        x = x.view(B, Lp, D)
        pooled = ln(x[:, 0].contiguous(), vm.post_layernorm, "post")
        wp = ck.get("proj", [self.visual_projection.weight], lambda: _bf(self.visual_projection.weight))
        return {"image_embeds": ops.linear(pooled, wp), "last_hidden_state": x[:, :L].contiguous()}


def read_clip_vision(path: str) -> ClipVisionNative:
    """a local HF directory (config.json + *.safetensors of CLIPVisionModelWithProjection or CLIPModel) or one .safetensors file (the
    ViT-L/14 geometry) -> ClipVisionNative with its weights (host memory)"""
    return _read_tower(path, ClipVisionNative, "CLIP vision")
