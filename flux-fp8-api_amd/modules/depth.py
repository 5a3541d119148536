"""A depth map from a photo on MI355X -- Depth Anything (V1 and V2; Small / Base / Large, relative depth), the estimator BFL's FLUX.1 Depth
pipeline runs (`LiheYoung/depth-anything-large-hf`) and the one behind the depth mode of the Union ControlNets.

The model is transformers' `DepthAnythingForDepthEstimation`, kept here in one place:
  1. backbone = DINOv2 (`Dinov2Backbone`): a stride-14 "valid" Conv2d(3, D, 14) on pixel_values [B, 3, 14 gh, 14 gw]; a class token in front;
     + the position embedding, whose patch rows are resized from the checkpoint's grid (37 x 37) to gh x gw -- bicubic, align_corners=False,
     in fp32 (`Dinov2Embeddings.interpolate_pos_encoding`; the table itself when the grid is the checkpoint's).  Pre-LN layers with
     LayerScale:  x += l1 * attn(LN(x));  x += l2 * fc2(gelu(fc1(LN(x)))), the exact (erf) GELU, heads of 64, scale 64^-1/2, LayerNorm eps
     1e-6 with bias.  The hidden states behind the layers `out_indices` go through the final `layernorm` (apply_layernorm) and lose the class row.
  2. neck, reassemble: per tapped state a 1 x 1 projection to neck_hidden_sizes[i] on the gh x gw grid, then by reassemble_factors
     [4, 2, 1, 0.5]: ConvTranspose2d(kernel = stride = 4), ConvTranspose2d(kernel = stride = 2), identity, Conv2d(3, stride 2, padding 1) --
     maps of 4g, 2g, g and ceil(g / 2); then a bias-free 3 x 3 convolution to fusion_hidden_size each (`neck.convs`).
  3. neck, fusion, from the smallest map up: h = f3;  then per layer  h = h + RCU1(f)  (not in the first),  h = RCU2(h),  h = bilinear
     resize with align_corners=True to the next map's size (x 2 behind the last),  h = 1 x 1 projection;  RCU(x) = x + conv(relu(conv(relu(x)))),
     the pre-activation residual unit.  In this model every fused state already has the size of the map it meets (the resize before it took
     that size explicitly), so the `align_corners=False` resize of the residual in transformers' DepthAnythingFeatureFusionLayer is never
     reached; it is not implemented.  `fusion_stage.layers.0.residual_layer1` is in the checkpoint and unused, as in transformers.
  4. head: 3 x 3 convolution to fusion / 2 at 8g, bilinear align_corners=True to (14 gh, 14 gw), 3 x 3 convolution to head_hidden_size +
     ReLU, 1 x 1 convolution to one channel + ReLU -> predicted_depth [B, 14 gh, 14 gw] (times max_depth = 1).

On libfluxmi: the tower is the SigLIP / CLIP towers' scheme (modules/encoder_common.py: fluxmi_patchify_rect + the bf16 GEMM,
fluxmi_row_norm, q | k as one GEMM, V^T from the swapped v-projection, fluxmi_vision_attention at head width 64) with LayerScale as the gate
of the GEMM's gate * y + x epilogue, where those towers pass ones, and fluxmi_unary for the exact GELU.  The decoder is NHWC bf16 throughout:
1 x 1 convolutions are GEMMs on the pixel rows; a ConvTranspose with kernel = stride = f is a GEMM to f * f * C' columns (row order
(i, j, c')) and a pixel shuffle (a torch permute copy); stride-1 3 x 3 convolutions run on fluxmi_conv3x3 (any H x W: its tests walk odd
grids and ragged tiles), the residual unit's sum in its gate * y + x epilogue; the stride-2 one is fluxmi_im2col3x3_s2 + the GEMM; ReLU =
fluxmi_unary; resizes = fluxmi_resize_bilinear; the head's 32-channel convolution + ReLU = fluxmi_conv3x3_dense with slope 0, its last
convolution + ReLU = fluxmi_depth_head, which keeps fp32.  So that the kernels' shape rules hold, channels are zero-padded once at load
(exact: a zero channel stays zero through ReLU, convolution, resize and sum, and zero weights drop it):
  * neck_hidden_sizes, fusion_hidden_size and the head's first width (fusion / 2) to multiples of 128 (fluxmi_conv3x3: C % 64 == 0, Cout %
    128 == 0; the GEMM's 128-column tiles).  Depth Anything Large (256 / 512 / 1024 / 1024, 256, 128) needs none;
  * head_hidden_size to a multiple of 32 (fluxmi_conv3x3_dense: Cout32 weight rows; <= 64 channels per launch, so 96 takes two);
  * heads narrower than 64 to 64, fc1 / fc2 to a multiple of 256, the patch matrix's K from 588 to 640, a sequence of gh gw + 1 tokens to
    a multiple of 256 rows (as for SigLIP / CLIP).
`padded_state_dict()` is that padded model in transformers' own key layout (tests/depth_ref.py runs it as it runs the checkpoint).
"""
from __future__ import annotations

import json
import os
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor, nn

from modules.conditioner import _bf, _Cache, _lin, _read_dir_weights
from modules.encoder_common import DINOV2_LAYER, encoder_layer, layer_weights, normalize_image, patch_embed, vision_attend
from modules.image_embedders import _pad_to, _round_up, to_pil

PATCH = 14
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)  # DPTImageProcessor's image_mean / image_std of the checkpoints
DEPTH_RES_MIN, DEPTH_RES_MAX = 14, 1036
# the longest sequence the attention kernel is checked at for this model (tests/test_depth_gpu.py): a 74 x 74 grid + the class token
MAX_TOKENS = 74 * 74 + 1

# keys left out of a config mean DepthAnythingConfig's / Dinov2Config's defaults, as transformers reads them
_DA_DEFAULTS = dict(patch_size=14, reassemble_hidden_size=384, reassemble_factors=[4, 2, 1, 0.5], neck_hidden_sizes=[48, 96, 192, 384],
                    fusion_hidden_size=64, head_in_index=-1, head_hidden_size=32, depth_estimation_type="relative", max_depth=None)
_DINOV2_DEFAULTS = dict(model_type="dinov2", hidden_size=768, num_hidden_layers=12, num_attention_heads=12, mlp_ratio=4, hidden_act="gelu",
                        layer_norm_eps=1e-6, image_size=224, patch_size=14, num_channels=3, qkv_bias=True, layerscale_value=1.0,
                        use_swiglu_ffn=False, out_features=None, out_indices=None, apply_layernorm=True, reshape_hidden_states=True,
                        use_mask_token=True)
# what DepthAnythingConfig builds when a config has no backbone_config at all
_DA_DEFAULT_BACKBONE = dict(image_size=518, hidden_size=384, num_attention_heads=6, out_indices=[9, 10, 11, 12], apply_layernorm=True,
                            reshape_hidden_states=False)


def depth_input_size(width: int, height: int, resolution: int = 518):
    """(width, height) the estimator sees for an image of width x height: DPTImageProcessor's resize with size = resolution x resolution,
    keep_aspect_ratio=True, ensure_multiple_of=14, as the Depth Anything checkpoints configure it.  Both scales resolution / side are
    formed, the one closer to 1 is applied to both sides ("scale as little as possible"), and each side goes to the nearest multiple of 14
    (Python's round: ties to even).  For the usual photo that makes the shorter side `resolution`; a side that would round to 0 becomes 14."""
    sh, sw = resolution / height, resolution / width
    if abs(1 - sw) < abs(1 - sh):
        sh = sw
    else:
        sw = sh
    return max(round(sw * width / PATCH), 1) * PATCH, max(round(sh * height / PATCH), 1) * PATCH


def interpolate_position_embedding(pos: Tensor, gh: int, gw: int) -> Tensor:
    """Dinov2Embeddings.interpolate_pos_encoding on the host: pos [1, 1 + n^2, D] -> [1 + gh gw, D] in pos's dtype; the patch rows through
    fp32, a bicubic align_corners=False resize and back; the table itself when the grid is the checkpoint's."""
    n = pos.shape[1] - 1
    s = int(n ** 0.5)
    if gh * gw == n and gh == gw:
        return pos[0]
    D = pos.shape[-1]
    grid = pos[:, 1:].reshape(1, s, s, D).permute(0, 3, 1, 2).to(torch.float32)
    grid = F.interpolate(grid, size=(gh, gw), mode="bicubic", align_corners=False).to(pos.dtype)
    return torch.cat((pos[0, :1], grid.permute(0, 2, 3, 1).reshape(gh * gw, D)), 0)


def resolve_config(config: Optional[dict]) -> dict:
    """a DepthAnythingConfig dict (config.json) with transformers' defaults filled in; refuses by name what the native model does not cover"""
    c = dict(_DA_DEFAULTS)
    c.update({k: v for k, v in (config or {}).items() if k != "backbone_config"})
    bc = dict(_DINOV2_DEFAULTS)
    raw = (config or {}).get("backbone_config")
    if raw is None:
        if (config or {}).get("backbone") is not None:
            raise ValueError(f"fluxmi: the native Depth Anything needs an inline backbone_config, not backbone={config['backbone']!r} (nothing is downloaded)")
        raw = _DA_DEFAULT_BACKBONE
    bc.update(raw)
    c["backbone_config"] = bc
    if bc.get("model_type", "dinov2") != "dinov2":
        raise ValueError(f"fluxmi: the native Depth Anything covers a DINOv2 backbone, got model_type={bc['model_type']!r}")
    if c["depth_estimation_type"] != "relative":
        raise ValueError(f"fluxmi: the native Depth Anything covers relative depth, got depth_estimation_type={c['depth_estimation_type']!r} "
                         "(metric checkpoints end in a sigmoid x max_depth)")
    if bc["use_swiglu_ffn"]:
        raise ValueError("fluxmi: the native Depth Anything covers the GELU MLP, got use_swiglu_ffn=True (DINOv2 giant)")
    if bc["hidden_act"] != "gelu":
        raise ValueError(f"fluxmi: the native Depth Anything covers hidden_act='gelu' (the exact GELU), got {bc['hidden_act']!r}")
    if bc["reshape_hidden_states"]:
        raise ValueError("fluxmi: the native Depth Anything reads token sequences: reshape_hidden_states=True is not covered (the checkpoints set False)")
    if c["head_hidden_size"] > 96:
        raise ValueError(f"fluxmi: head_hidden_size={c['head_hidden_size']} is above 96, the widest head the dense convolution kernel is run at")
    D, H = bc["hidden_size"], bc["num_attention_heads"]
    if D % H or D % 128 or D // H > 64:
        raise ValueError(f"fluxmi: DINOv2 hidden_size {D} must be a multiple of 128 and of the head count {H}, with heads of at most 64")
    if bc["patch_size"] != PATCH or c["patch_size"] != PATCH or bc["num_channels"] != 3 or not bc["qkv_bias"]:
        raise ValueError("fluxmi: the native Depth Anything covers patch_size 14, 3 channels and qkv_bias=True")
    if c["reassemble_hidden_size"] != D:
        raise ValueError(f"fluxmi: reassemble_hidden_size {c['reassemble_hidden_size']} must equal the backbone's hidden_size {D}")
    fac = [float(f) for f in c["reassemble_factors"]]
    if len(fac) != len(c["neck_hidden_sizes"]) or any(f not in (4.0, 2.0, 1.0, 0.5) for f in fac):
        raise ValueError(f"fluxmi: reassemble_factors {c['reassemble_factors']} must be one of 4, 2, 1, 0.5 per neck_hidden_sizes entry")
    # the fusion stage meets each map at the size the previous resize took: consecutive maps must not shrink (the checkpoints' 4, 2, 1, 0.5)
    if any(a < b for a, b in zip(fac, fac[1:])):
        raise ValueError(f"fluxmi: reassemble_factors {c['reassemble_factors']} must not increase")
    if c["head_in_index"] not in (-1, len(fac) - 1):
        raise ValueError(f"fluxmi: head_in_index={c['head_in_index']} must select the last fused state")
    if c["fusion_hidden_size"] % 2 or _round_up(c["fusion_hidden_size"] // 2, 128) > 256:
        raise ValueError(f"fluxmi: fusion_hidden_size={c['fusion_hidden_size']} must be even and at most 512 (the head's dense convolution reads <= 256 channels)")
    idx = bc["out_indices"]
    if idx is None:
        idx = [int(s[len("stage"):]) for s in bc["out_features"]] if bc["out_features"] is not None else [bc["num_hidden_layers"]]
    idx = [int(i) for i in idx]
    if len(idx) != len(fac) or any(not 1 <= i <= bc["num_hidden_layers"] for i in idx) or sorted(idx) != idx:
        raise ValueError(f"fluxmi: out_indices {idx} must name {len(fac)} layers in 1..{bc['num_hidden_layers']}, ascending")
    bc["out_indices"] = idx
    return c


class _Dinov2Backbone(nn.Module):
    def __init__(self, bc):
        super().__init__()
        D, Fd, n = bc["hidden_size"], int(bc["hidden_size"] * bc["mlp_ratio"]), (bc["image_size"] // PATCH) ** 2
        self.embeddings = nn.Module()
        self.embeddings.cls_token = nn.Parameter(torch.zeros(1, 1, D), requires_grad=False)
        self.embeddings.position_embeddings = nn.Parameter(torch.zeros(1, n + 1, D), requires_grad=False)
        self.embeddings.patch_embeddings = nn.Module()
        self.embeddings.patch_embeddings.projection = nn.Conv2d(3, D, kernel_size=PATCH, stride=PATCH)
        self.encoder = nn.Module()
        self.encoder.layer = nn.ModuleList()
        for _ in range(bc["num_hidden_layers"]):
            lay = nn.Module()
            lay.norm1, lay.norm2 = nn.LayerNorm(D, eps=bc["layer_norm_eps"]), nn.LayerNorm(D, eps=bc["layer_norm_eps"])
            lay.attention = nn.Module()
            lay.attention.attention = nn.Module()
            for n_ in ("query", "key", "value"):
                setattr(lay.attention.attention, n_, _lin(D, D, True))
            lay.attention.output = nn.Module()
            lay.attention.output.dense = _lin(D, D, True)
            lay.layer_scale1, lay.layer_scale2 = nn.Module(), nn.Module()
            lay.layer_scale1.lambda1 = nn.Parameter(torch.ones(D), requires_grad=False)
            lay.layer_scale2.lambda1 = nn.Parameter(torch.ones(D), requires_grad=False)
            lay.mlp = nn.Module()
            lay.mlp.fc1, lay.mlp.fc2 = _lin(D, Fd, True), _lin(Fd, D, True)
            self.encoder.layer.append(lay)
        self.layernorm = nn.LayerNorm(D, eps=bc["layer_norm_eps"])
        self.requires_grad_(False)


class _Neck(nn.Module):
    def __init__(self, c):
        super().__init__()
        D, Fh = c["reassemble_hidden_size"], c["fusion_hidden_size"]
        self.reassemble_stage = nn.Module()
        self.reassemble_stage.layers = nn.ModuleList()
        self.convs = nn.ModuleList()
        self.fusion_stage = nn.Module()
        self.fusion_stage.layers = nn.ModuleList()
        for ch, f in zip(c["neck_hidden_sizes"], c["reassemble_factors"]):
            lay = nn.Module()
            lay.projection = nn.Conv2d(D, ch, 1)
            if f > 1:
                lay.resize = nn.ConvTranspose2d(ch, ch, kernel_size=int(f), stride=int(f))
            elif f < 1:
                lay.resize = nn.Conv2d(ch, ch, 3, stride=int(round(1 / f)), padding=1)
            self.reassemble_stage.layers.append(lay)
            self.convs.append(nn.Conv2d(ch, Fh, 3, padding=1, bias=False))
            fus = nn.Module()
            fus.projection = nn.Conv2d(Fh, Fh, 1)
            for n in ("residual_layer1", "residual_layer2"):
                rcu = nn.Module()
                rcu.convolution1, rcu.convolution2 = nn.Conv2d(Fh, Fh, 3, padding=1), nn.Conv2d(Fh, Fh, 3, padding=1)
                setattr(fus, n, rcu)
            self.fusion_stage.layers.append(fus)
        self.requires_grad_(False)


class DepthAnythingNative(nn.Module):
    """State-dict keys of transformers' DepthAnythingForDepthEstimation (backbone.embeddings.{cls_token, position_embeddings,
    patch_embeddings.projection}, backbone.encoder.layer.{i}.{norm1, attention.attention.{query,key,value}, attention.output.dense,
    layer_scale1.lambda1, norm2, mlp.{fc1,fc2}, layer_scale2.lambda1}, backbone.layernorm, neck.reassemble_stage.layers.{i}.{projection,
    resize}, neck.convs.{i}, neck.fusion_stage.layers.{i}.{projection, residual_layer{1,2}.convolution{1,2}}, head.conv{1,2,3}), loaded
    strict; backbone.embeddings.mask_token is ignored.  `config`: the checkpoint's config.json as a dict (see resolve_config for what is
    refused); None = transformers' default DepthAnythingConfig.  forward: pixel_values [B, 3, 14 gh, 14 gw] -> predicted_depth fp32
    [B, 14 gh, 14 gw] for any gh, gw >= 1 with gh gw + 1 <= MAX_TOKENS."""

    def __init__(self, config: Optional[dict] = None):
        super().__init__()
        c = self.cfg = resolve_config(config)
        bc = c["backbone_config"]
        self.head_dim = bc["hidden_size"] // bc["num_attention_heads"]
        self.backbone = _Dinov2Backbone(bc)
        self.neck = _Neck(c)
        Fh = c["fusion_hidden_size"]
        self.head = nn.Module()
        self.head.conv1 = nn.Conv2d(Fh, Fh // 2, 3, padding=1)
        self.head.conv2 = nn.Conv2d(Fh // 2, c["head_hidden_size"], 3, padding=1)
        self.head.conv3 = nn.Conv2d(c["head_hidden_size"], 1, 1)
        self.requires_grad_(False)
        self._cache = _Cache()

    def load_state_dict(self, sd, strict=True, assign=False):
        return super().load_state_dict({k: v for k, v in sd.items() if not k.endswith("embeddings.mask_token")}, strict=strict, assign=assign)

    @property
    def device(self):
        return self.backbone.layernorm.weight.device

    @property
    def mlp_pad(self) -> int:
        bc = self.cfg["backbone_config"]
        return _round_up(int(bc["hidden_size"] * bc["mlp_ratio"]), 256)

    @property
    def patch_k(self) -> int:
        return _round_up(3 * PATCH * PATCH, 64)

    def seq_pad(self, gh: int, gw: int) -> int:
        return _round_up(gh * gw + 1, 256)

    # ---- padded weights ----------------------------------------------------------------------------------------------------------------
    def padded_sizes(self) -> dict:
        c = self.cfg
        return dict(neck=[_round_up(n, 128) for n in c["neck_hidden_sizes"]], fusion=_round_up(c["fusion_hidden_size"], 128),
                    head1=_round_up(c["fusion_hidden_size"] // 2, 128), head=_round_up(c["head_hidden_size"], 32))

    def padded_state_dict(self) -> dict:
        """the neck's and the head's weights zero-padded to padded_sizes(), in transformers' key layout and the parameters' dtype (the
        backbone's keys unchanged): the model the decoder kernels run, as a checkpoint tests/depth_ref.py can run too"""
        ps = self.padded_sizes()
        sd = {k: v.detach() for k, v in self.state_dict().items()}

        def pad(key, *dims):  # dims: the padded size of each leading dim (None = keep)
            t = sd[key]
            for d, n in enumerate(dims):
                if n is not None:
                    t = _pad_to(t, n, d)
            sd[key] = t.contiguous()

        Fp = ps["fusion"]
        for i, Np in enumerate(ps["neck"]):
            p = f"neck.reassemble_stage.layers.{i}."
            pad(p + "projection.weight", Np)
            pad(p + "projection.bias", Np)
            if p + "resize.weight" in sd:
                pad(p + "resize.weight", Np, Np)
                pad(p + "resize.bias", Np)
            pad(f"neck.convs.{i}.weight", Fp, Np)
            q = f"neck.fusion_stage.layers.{i}."
            pad(q + "projection.weight", Fp, Fp)
            pad(q + "projection.bias", Fp)
            for n in ("residual_layer1", "residual_layer2"):
                for m in ("convolution1", "convolution2"):
                    pad(f"{q}{n}.{m}.weight", Fp, Fp)
                    pad(f"{q}{n}.{m}.bias", Fp)
        pad("head.conv1.weight", ps["head1"], Fp)
        pad("head.conv1.bias", ps["head1"])
        pad("head.conv2.weight", ps["head"], ps["head1"])
        pad("head.conv2.bias", ps["head"])
        pad("head.conv3.weight", None, ps["head"])
        return sd

    def _kernel_weights(self) -> dict:
        """bf16 weights of the neck and the head in the layouts the kernels take, from padded_state_dict(), built once"""

        def build():
            sd = self.padded_state_dict()
            k = {}
            w3 = lambda t: _bf(t).permute(0, 2, 3, 1).reshape(t.shape[0], -1).contiguous()  # noqa: E731  [Cout, Cin, 3, 3] -> [Cout, (dy, dx, c)]
            for i, f in enumerate(self.cfg["reassemble_factors"]):
                p = f"neck.reassemble_stage.layers.{i}."
                k[f"proj{i}.w"], k[f"proj{i}.b"] = _bf(sd[p + "projection.weight"]).flatten(1).contiguous(), _bf(sd[p + "projection.bias"])
                if f > 1:  # ConvTranspose weight [Cin, Cout, f, f] -> GEMM rows (i, j, cout), bias repeated per (i, j)
                    w = _bf(sd[p + "resize.weight"])
                    k[f"up{i}.w"] = w.permute(2, 3, 1, 0).reshape(-1, w.shape[0]).contiguous()
                    k[f"up{i}.b"] = _bf(sd[p + "resize.bias"]).repeat(int(f) * int(f)).contiguous()
                elif f < 1:
                    k[f"down{i}.w"], k[f"down{i}.b"] = w3(sd[p + "resize.weight"]), _bf(sd[p + "resize.bias"])
                k[f"conv{i}.w"] = w3(sd[f"neck.convs.{i}.weight"])
                q = f"neck.fusion_stage.layers.{i}."
                k[f"fproj{i}.w"], k[f"fproj{i}.b"] = _bf(sd[q + "projection.weight"]).flatten(1).contiguous(), _bf(sd[q + "projection.bias"])
                for n, tag in (("residual_layer1", "r1"), ("residual_layer2", "r2")):
                    for m, t2 in (("convolution1", "c1"), ("convolution2", "c2")):
                        k[f"{tag}{t2}{i}.w"], k[f"{tag}{t2}{i}.b"] = w3(sd[f"{q}{n}.{m}.weight"]), _bf(sd[f"{q}{n}.{m}.bias"])
            k["head1.w"], k["head1.b"] = w3(sd["head.conv1.weight"]), _bf(sd["head.conv1.bias"])
            k["head2.w"] = _bf(sd["head.conv2.weight"]).permute(0, 2, 3, 1).contiguous()  # [Cout32, 3, 3, Cin]
            k["head2.b"] = _bf(sd["head.conv2.bias"])
            k["head3.w"], k["head3.b"] = _bf(sd["head.conv3.weight"]).reshape(-1).contiguous(), _bf(sd["head.conv3.bias"])
            k["ones"] = torch.ones(self.padded_sizes()["fusion"], dtype=torch.bfloat16, device=sd["head.conv3.bias"].device)
            return k

        return self._cache.get("decoder", list(self.neck.parameters()) + list(self.head.parameters()), build)

    def layer_weights(self, i) -> dict:
        """bf16 weights of backbone layer i (or i = "embed") as the kernels take them, built once"""
        bb, ck = self.backbone, self._cache
        bc = self.cfg["backbone_config"]
        if i == "embed":
            pe = bb.embeddings.patch_embeddings.projection
            return dict(w=ck.get("patch_w", [pe.weight], lambda: _pad_to(_bf(pe.weight).reshape(pe.weight.shape[0], -1), self.patch_k, 1).contiguous()),
                        b=ck.get("patch_b", [pe.bias], lambda: _bf(pe.bias)))
        return layer_weights(ck, bb.encoder.layer[i], DINOV2_LAYER, i, bc["num_attention_heads"], self.head_dim, 64, self.mlp_pad)

    def position_rows(self, gh: int, gw: int):
        """(class row bf16 [D] = bf16(cls_token + pos[0]), patch rows bf16 [gh gw, D]) on the model's device; interpolated once per grid on the
        host, through fp32 from the bf16 values of the table as transformers' bf16 model does, then cached"""
        em = self.backbone.embeddings

        def build():
            pos = interpolate_position_embedding(_bf(em.position_embeddings).cpu(), gh, gw).to(em.position_embeddings.device)
            return torch.cat(((_bf(em.cls_token)[0, 0] + pos[0])[None], pos[1:]), 0).contiguous()

        rows = self._cache.get(("pos", gh, gw), [em.position_embeddings, em.cls_token], build)
        return rows[0], rows[1:]

    # ---- forward -----------------------------------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def features(self, pixel_values: Tensor) -> list:
        """the backbone: pixel_values [B, 3, 14 gh, 14 gw] -> the tapped hidden states, each bf16 [B, gh, gw, D] (NHWC, dense)"""
        from fluxmi import ops

        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("fluxmi: the Depth Anything estimator needs the GPU (libfluxmi has no CPU path)")
        bc, ck, bb = self.cfg["backbone_config"], self._cache, self.backbone
        D, H, eps = bc["hidden_size"], bc["num_attention_heads"], bc["layer_norm_eps"]
        pix = pixel_values.to(device=dev, dtype=torch.bfloat16)
        if pix.dim() != 4 or pix.shape[1] != 3 or pix.shape[2] < PATCH or pix.shape[3] < PATCH or pix.shape[2] % PATCH or pix.shape[3] % PATCH:
            raise ValueError(f"fluxmi: Depth Anything takes pixel_values [B, 3, 14 gh, 14 gw] with gh, gw >= 1, got {tuple(pixel_values.shape)}")
        B, gh, gw = pix.shape[0], pix.shape[2] // PATCH, pix.shape[3] // PATCH
        L, Lp = gh * gw + 1, self.seq_pad(gh, gw)
        if L > MAX_TOKENS:
            raise ValueError(f"fluxmi: a {gh} x {gw} patch grid is {L} tokens, above the {MAX_TOKENS} the estimator is checked at (74 x 74 + 1): "
                             "lower the resolution")
        ones = ck.get("ones", [bb.layernorm.weight], lambda: torch.ones(D, dtype=torch.bfloat16, device=dev))
        cls_row, pos_rows = self.position_rows(gh, gw)
        # row 0 of each image's Lp-row slab: the class row; rows 1 .. G: bf16(pos + bf16(conv)); the rest zero (finite through every layer)
        e = self.layer_weights("embed")
        x = patch_embed(pix, PATCH, gh, gw, self.patch_k, e["w"], e["b"], pos_rows, cls_row, Lp, ones)
        g_f, e_f = (ck.get((n, "final"), [t], lambda t=t: _bf(t)) for n, t in (("g", bb.layernorm.weight), ("e", bb.layernorm.bias)))
        attend, gelu = vision_attend(B, L, Lp, H, self.head_dim, 64), lambda f: ops.unary(f, "gelu", out=f)  # noqa: E731
        taps = []
        for i in range(max(bc["out_indices"])):
            p = self.layer_weights(i)
            # LayerScale: x + lambda * (y W^T + b) is the gate * y + x epilogue with the gate lambda
            x = encoder_layer(x, p, attend, gelu, eps, p["l1"], p["l2"])
            if i + 1 in bc["out_indices"]:
                y = ops.row_norm(x, g_f, e_f, eps=eps, rms=False) if bc["apply_layernorm"] else x
                taps.append(y.view(B, Lp, D)[:, 1:L].reshape(B, gh, gw, D))
        return taps

    @staticmethod
    def _rcu(x: Tensor, k: dict, unit: str, j: int) -> Tensor:
        """the pre-activation residual unit `unit` ("r1" / "r2") of fusion layer j: x + conv2(relu(conv1(relu(x)))) on [B, H, W, Fp]"""
        from fluxmi import ops

        h = ops.conv3x3(ops.unary(x, "relu"), k[f"{unit}c1{j}.w"], k[f"{unit}c1{j}.b"])
        ops.unary(h, "relu", out=h)
        return ops.conv3x3(h, k[f"{unit}c2{j}.w"], k[f"{unit}c2{j}.b"], resid=x, gate=k["ones"])

    @torch.inference_mode()
    def decode(self, taps: list) -> Tensor:
        """the neck and the head: tapped states [B, gh, gw, D] bf16 -> predicted_depth fp32 [B, 14 gh, 14 gw]"""
        from fluxmi import ops

        c, k, ps = self.cfg, self._kernel_weights(), self.padded_sizes()
        B, gh, gw, D = taps[0].shape
        feats = []
        for i, (t, f) in enumerate(zip(taps, c["reassemble_factors"])):
            Np = ps["neck"][i]
            x = ops.linear(t.reshape(B * gh * gw, D), k[f"proj{i}.w"], k[f"proj{i}.b"])
            if f > 1:
                f = int(f)
                y = ops.linear(x, k[f"up{i}.w"], k[f"up{i}.b"])  # [B gh gw, (i, j, c)]
                x = y.view(B, gh, gw, f, f, Np).permute(0, 1, 3, 2, 4, 5).reshape(B, gh * f, gw * f, Np)  # the pixel shuffle (a copy)
            elif f < 1:
                x = ops.conv3x3_s2(x.view(B, gh, gw, Np), k[f"down{i}.w"], k[f"down{i}.b"])
            else:
                x = x.view(B, gh, gw, Np)
            feats.append(ops.conv3x3(x, k[f"conv{i}.w"]))
        feats = feats[::-1]
        fused = None
        for j, f in enumerate(feats):
            fused = f if fused is None else ops.add(fused, self._rcu(f, k, "r1", j))
            fused = self._rcu(fused, k, "r2", j)
            size = tuple(feats[j + 1].shape[1:3]) if j + 1 < len(feats) else (2 * fused.shape[1], 2 * fused.shape[2])
            up = ops.resize_bilinear(fused, size)
            fused = ops.linear(up.view(-1, ps["fusion"]), k[f"fproj{j}.w"], k[f"fproj{j}.b"]).view(B, size[0], size[1], ps["fusion"])
        x = ops.conv3x3(fused, k["head1.w"], k["head1.b"])
        x = ops.resize_bilinear(x, (PATCH * gh, PATCH * gw))
        hidden = torch.empty(B, PATCH * gh, PATCH * gw, ps["head"], dtype=torch.bfloat16, device=x.device)
        for c0 in range(0, ps["head"], 64):  # <= 64 output channels per launch; the ReLU is the leaky ReLU at slope 0
            n = min(64, ps["head"] - c0)
            ops.conv3x3_dense(x, k["head2.w"][c0:c0 + n], k["head2.b"][c0:c0 + n], hidden[..., c0:c0 + n], slope=0.0, act=True)
        return ops.depth_head(hidden, k["head3.w"], k["head3.b"])

    @torch.inference_mode()
    def forward(self, pixel_values: Tensor, **_) -> Tensor:
        """pixel_values [B, 3, 14 gh, 14 gw] -> predicted_depth fp32 [B, 14 gh, 14 gw]"""
        return self.decode(self.features(pixel_values))

    # ---- photo -> depth -------------------------------------------------------------------------------------------------------------------
    def preprocess(self, image, resolution: int = 518) -> Tensor:
        """DPTImageProcessor as the checkpoints configure it -> fp32 [1, 3, 14 gh, 14 gw] on the host: RGB, PIL bicubic resize to
        depth_input_size, x / 255, ImageNet mean / std.  `image`: anything to_pil takes."""
        from PIL import Image

        pil = to_pil(image).convert("RGB")
        size = depth_input_size(pil.width, pil.height, resolution)
        if size != pil.size:
            pil = pil.resize(size, resample=Image.BICUBIC)
        return normalize_image(np.asarray(pil), IMAGENET_MEAN, IMAGENET_STD)

    @torch.inference_mode()
    def depth_map(self, image, size=None, resolution: int = 518, normalize: str = "minmax") -> Tensor:
        """a photo -> its depth map uint8 [H, W, 3] on the model's device (near = bright, the form FLUX.1 Depth and the depth ControlNets
        take): preprocess, the model, fluxmi_depth_to_map to size = (H, W) (default: the photo's own)."""
        from fluxmi import ops

        pil = to_pil(image)
        H, W = (pil.height, pil.width) if size is None else (int(size[0]), int(size[1]))
        depth = self(self.preprocess(pil, resolution).to(self.device))
        return ops.depth_to_map(depth, (H, W), normalize)[0]


def read_depth_anything(path: str) -> DepthAnythingNative:
    """a local HF directory (config.json + model.safetensors / *.safetensors, or pytorch_model.bin) of DepthAnythingForDepthEstimation ->
    DepthAnythingNative with its weights (host memory).  Nothing is downloaded."""
    if not os.path.isdir(path):
        raise FileNotFoundError(f"fluxmi: depth_path {path!r} must be a local directory holding config.json and the weights")
    cj = os.path.join(path, "config.json")
    if not os.path.exists(cj):
        raise FileNotFoundError(f"fluxmi: no config.json under {path} (the Depth Anything geometry is read from it)")
    with open(cj) as f:
        cfg = json.load(f)
    if any(f.endswith(".safetensors") for f in os.listdir(path)):
        sd = _read_dir_weights(path)
    else:
        bins = sorted(f for f in os.listdir(path) if f.endswith(".bin"))
        if not bins:
            raise FileNotFoundError(f"fluxmi: no *.safetensors or *.bin weights under {path}")
        sd = {}
        for b in bins:
            sd.update(torch.load(os.path.join(path, b), map_location="cpu", weights_only=True))
    m = DepthAnythingNative(cfg)
    m.load_state_dict(sd, strict=True)
    return m
