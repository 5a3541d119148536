"""FLUX ControlNet (diffusers' `FluxControlNetModel`: the InstantX / Shakker-Labs Canny, Depth, Union, Union-Pro, Union-Pro-2.0 checkpoints)
as a parameter container over the native engine, like modules/flux_model.py.

A ControlNet is a short Flux trunk with its own embedders and no final layer, plus `controlnet_x_embedder` (the control latent joins the
image stream in front of block 0), one `controlnet_blocks[k]` / `controlnet_single_blocks[k]` projection behind every block and, for a
Union net, `controlnet_mode_embedder` (one more text token).  The modules carry BFL-style names (img_in, double_blocks[i].img_attn.qkv, ...)
so that float8_quantize and the engine's layer table treat the trunk exactly like Flux's; `convert_diffusers_controlnet_checkpoint` renames a
diffusers checkpoint.  The net never runs alone: `Flux.forward` / `Flux.denoise` take `controlnet=ControlNetCall(net, cond, scale, mode)` and
the engine runs both block stacks inside one step (csrc/engine.hip, fluxmi_engine_attach_controlnet).
"""
from __future__ import annotations

import ctypes as C
import math
import re
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch
from torch import Tensor, nn

from fluxmi import _lib, ops
from modules.flux_model import Flux


# ---- which steps of a schedule a ControlNet is applied to, which residual a main block takes ---------------------------------------------
def control_steps(n_steps: int, start: float = 0.0, end: float = 1.0) -> List[bool]:
    """diffusers' controlnet_keep: step i of n uses the ControlNet iff not (i / n < start or (i + 1) / n > end)."""
    return [not (i / n_steps < start or (i + 1) / n_steps > end) for i in range(n_steps)]


def residual_index(i: int, n_blocks: int, n_residuals: int) -> int:
    """FluxTransformer2DModel.forward: block i of n_blocks adds residual i // ceil(n_blocks / n_residuals)."""
    return i // int(math.ceil(n_blocks / n_residuals))


# ---- diffusers key names -> BFL-style names ----------------------------------------------------------------------------------------------
def _name_tables():
    """(top, double, single) tables of (diffusers stem, BFL stem): the tables behind lora_loading.convert_diffusers_to_flux_transformer_checkpoint
    plus the entries a full checkpoint has and a LoRA file does not; a BFL stem that ends in `.scale` is an RMSNorm weight."""
    import lora_loading as ll

    top = [(a, b) for a, b, _ in ll._DIFFUSERS_TOP] + [("time_text_embed.timestep_embedder.linear_2", "time_in.out_layer")]
    double = list(ll._DIFFUSERS_DOUBLE_PRE) + list(ll._DIFFUSERS_DOUBLE_POST)
    single = [("norm.linear", "modulation.lin"), ("proj_out", "linear2"), ("attn.norm_q", "norm.query_norm.scale"),
              ("attn.norm_k", "norm.key_norm.scale")]
    return top, double, single


def inspect_diffusers_controlnet(sd: Dict[str, Tensor]) -> dict:
    """Geometry of a diffusers FluxControlNetModel state dict, read off its keys: Nd, Ns, num_mode, guidance_embed (+ hidden, in_channels)."""
    if any(k.startswith("input_hint_block") for k in sd):
        raise ValueError("fluxmi: this checkpoint has an `input_hint_block` (the XLabs ControlNet format); only diffusers-format "
                         "FluxControlNetModel checkpoints (InstantX, Shakker-Labs) are supported")
    if "controlnet_x_embedder.weight" not in sd:
        raise ValueError("fluxmi: not a diffusers FluxControlNetModel checkpoint (no controlnet_x_embedder.weight)")
    count = lambda pat: len({int(m.group(1)) for k in sd for m in [re.match(pat, k)] if m})
    nd, ns = count(r"controlnet_blocks\.(\d+)\.weight$"), count(r"controlnet_single_blocks\.(\d+)\.weight$")
    if nd != count(r"transformer_blocks\.(\d+)\.norm1\.linear\.weight$") or ns != count(r"single_transformer_blocks\.(\d+)\.norm\.linear\.weight$"):
        raise ValueError("fluxmi: the checkpoint's controlnet_blocks / controlnet_single_blocks do not match its transformer blocks one to one "
                         "(diffusers' controlnet_blocks_repeat layouts are not supported)")
    if nd < 1:
        raise ValueError("fluxmi: a ControlNet needs at least one double block")
    mode = sd.get("controlnet_mode_embedder.weight")
    w = sd["controlnet_x_embedder.weight"]
    return dict(num_double=nd, num_single=ns, num_mode=0 if mode is None else int(mode.shape[0]),
                guidance_embed="time_text_embed.guidance_embedder.linear_1.weight" in sd, hidden_size=int(w.shape[0]), in_channels=int(w.shape[1]))


def convert_diffusers_controlnet_checkpoint(sd: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """diffusers FluxControlNetModel keys -> FluxControlNet's (BFL-style) keys.  q / k / v (single blocks: and proj_mlp) are concatenated into
    qkv / linear1, norm1.linear -> img_mod.lin and so on; there is no final layer, hence no (shift, scale) swap.  The input is not modified."""
    info = inspect_diffusers_controlnet(sd)
    top, double, single = _name_tables()
    out: Dict[str, Tensor] = {}
    used = set()

    def move(src: str, dst: str, required=True):
        if dst.endswith(".scale"):
            pairs = [(src + ".weight", dst)]
        else:
            pairs = [(src + ".weight", dst + ".weight"), (src + ".bias", dst + ".bias")]
        for i, (a, b) in enumerate(pairs):
            if a in sd:
                out[b] = sd[a]
                used.add(a)
            elif required and i == 0:
                raise KeyError(f"fluxmi: ControlNet checkpoint has no {a}")

    def fuse(srcs: List[str], dst: str):
        for suf in (".weight", ".bias"):
            keys = [s + suf for s in srcs]
            have = [k in sd for k in keys]
            if all(have):
                out[dst + suf] = torch.cat([sd[k] for k in keys], 0)
                used.update(keys)
            elif any(have) or suf == ".weight":
                raise KeyError(f"fluxmi: ControlNet checkpoint is missing {[k for k, h in zip(keys, have) if not h]}")

    for a, b in top:
        move(a, b, required=not b.startswith("guidance_in") or info["guidance_embed"])
    for i in range(info["num_double"]):
        dp, bp = f"transformer_blocks.{i}.", f"double_blocks.{i}."
        for a, b in double:
            move(dp + a, bp + b)
        fuse([dp + "attn." + c for c in ("to_q", "to_k", "to_v")], bp + "img_attn.qkv")
        fuse([dp + "attn." + c for c in ("add_q_proj", "add_k_proj", "add_v_proj")], bp + "txt_attn.qkv")
        move(f"controlnet_blocks.{i}", f"controlnet_blocks.{i}")
    for i in range(info["num_single"]):
        dp, bp = f"single_transformer_blocks.{i}.", f"single_blocks.{i}."
        for a, b in single:
            move(dp + a, bp + b)
        fuse([dp + "attn.to_q", dp + "attn.to_k", dp + "attn.to_v", dp + "proj_mlp"], bp + "linear1")
        move(f"controlnet_single_blocks.{i}", f"controlnet_single_blocks.{i}")
    move("controlnet_x_embedder", "controlnet_x_embedder")
    if info["num_mode"]:
        out["controlnet_mode_embedder.weight"] = sd["controlnet_mode_embedder.weight"]
        used.add("controlnet_mode_embedder.weight")
    left = sorted(set(sd) - used)
    if left:
        raise ValueError(f"fluxmi: ControlNet checkpoint has {len(left)} keys this converter does not know: {left[:6]}")
    return out


# ---- the module --------------------------------------------------------------------------------------------------------------------------
@dataclass
class ControlNetCall:
    """The `controlnet=` argument of Flux.forward / Flux.denoise: the net, the packed control latent `cond` [B, Li, in_channels] (VAE-encoded,
    shifted, scaled, packed: flux_pipeline.prepare_controlnet_conditioning) for the caller's B images, the conditioning scale (any float; it
    is never rounded to bf16) and, for a Union net, the control mode."""
    net: "FluxControlNet"
    cond: Tensor
    scale: float = 1.0
    mode: Optional[int] = None


class FluxControlNet(Flux):
    """diffusers' FluxControlNetModel over the engine: Flux's embedders and `num_double` + `num_single` blocks under their BFL names (quantised
    by the same flags), no final layer, and the bf16 `controlnet_*` projections.  `config`: the ModelSpec of the main model it steers."""

    def __init__(self, config, num_double: int, num_single: int, num_mode: int = 0, guidance_embed: Optional[bool] = None,
                 dtype: torch.dtype = torch.bfloat16):
        spec = config.model_copy(deep=True)
        p = spec.params
        if p.out_channels is not None and p.out_channels != p.in_channels:
            raise ValueError("fluxmi: FLUX.1 Fill / Depth / Canny [dev] models (in_channels != out_channels) take no ControlNet")
        if num_double < 1 or num_single < 0 or num_mode < 0:
            raise ValueError(f"fluxmi: ControlNet with {num_double} double / {num_single} single blocks, {num_mode} modes")
        p.depth, p.depth_single_blocks = int(num_double), int(num_single)
        if guidance_embed is not None:
            p.guidance_embed = bool(guidance_embed)
        super().__init__(spec, dtype=dtype)
        self.final_layer = None  # a ControlNet predicts nothing
        H = self.hidden_size
        self.controlnet_x_embedder = nn.Linear(self.in_channels, H)
        self.controlnet_blocks = nn.ModuleList([nn.Linear(H, H) for _ in range(num_double)])
        self.controlnet_single_blocks = nn.ModuleList([nn.Linear(H, H) for _ in range(num_single)])
        self.controlnet_mode_embedder = nn.Embedding(num_mode, H) if num_mode else None
        self.num_mode = int(num_mode)
        self.requires_grad_(False)

    @property
    def is_union(self) -> bool:
        return self.num_mode > 0

    def controlnet_linears(self) -> List[nn.Module]:
        return [self.controlnet_x_embedder] + list(self.controlnet_blocks) + list(self.controlnet_single_blocks)

    def linear_modules(self) -> List[nn.Module]:
        """The canonical order of include/fluxmi.h (fluxmi_controlnet_create): the trunk without a final layer, then the projections."""
        mods = [self.img_in, self.time_in.in_layer, self.time_in.out_layer, self.vector_in.in_layer, self.vector_in.out_layer]
        if self.params.guidance_embed:
            mods += [self.guidance_in.in_layer, self.guidance_in.out_layer]
        mods.append(self.txt_in)
        for b in self.double_blocks:
            for s in ("img", "txt"):
                a, m = getattr(b, f"{s}_attn"), getattr(b, f"{s}_mlp")
                mods += [getattr(b, f"{s}_mod").lin, a.qkv, a.proj, m[0], m[2]]
        for b in self.single_blocks:
            mods += [b.modulation.lin, b.linear1, b.linear2]
        return mods + self.controlnet_linears()

    def _desc(self):
        p = self.params
        d = _lib.ModelDesc()
        d.hidden, d.heads, d.mlp_hidden = p.hidden_size, p.num_heads, int(p.hidden_size * p.mlp_ratio)
        d.depth, d.depth_single, d.in_channels = p.depth, p.depth_single_blocks, p.in_channels
        d.vec_in, d.ctx_in, d.guidance_embed = p.vec_in_dim, p.context_in_dim, int(p.guidance_embed)
        d.axes_dim = (C.c_int * 3)(*p.axes_dim)
        d.theta = p.theta
        f8 = self.f8_modules()
        d.num_trials = f8[0].num_scale_trials if f8 else 12
        return d

    def _ensure_engine(self, device):
        if self._engine is not None:
            return
        if device.type != "cuda":
            raise RuntimeError("FluxControlNet (fluxmi): the model must run on a GPU; there is no CPU path")
        from float8_quantize import F8Linear

        if any(isinstance(m, F8Linear) for m in self.controlnet_linears()):
            raise ValueError("fluxmi: the controlnet_* projections stay bf16 nn.Linear (like final_layer); quantise the blocks only")
        p = self.params
        d = self._desc()
        lin, keep_l = self._linear_table(device)
        nrm, keep_n = self._norm_table(device)
        table = None
        if self.controlnet_mode_embedder is not None:
            table = self.controlnet_mode_embedder.weight.data.to(device=device, dtype=torch.bfloat16).contiguous()
        h = C.c_void_p()
        _lib.call("fluxmi_controlnet_create", C.byref(d), lin, len(lin), nrm, len(nrm), ops._p(table), self.num_mode, C.byref(h))
        om, ax = ops.rope_tables_host(p.axes_dim, p.theta)
        fr = ops.timestep_freqs_host(128)
        _lib.call("fluxmi_engine_set_tables", h, fr.numpy().ctypes.data_as(C.POINTER(C.c_float)),
                  om.numpy().ctypes.data_as(C.POINTER(C.c_float)), ax.numpy().ctypes.data_as(C.POINTER(C.c_int)))
        self._engine, self._engine_keep, self._prep_key, self._engine_device = h, (keep_l, keep_n, lin, nrm, table), None, device
        if self._amax_xchg is not None:
            self._install_amax_exchange()

    def rebind_weights(self):
        if self._engine is None:
            return
        lin, keep_l = self._linear_table(self._engine_device)
        with self._lock:
            _lib.call("fluxmi_engine_rebind", self._engine, lin, len(lin))
            self._engine_keep = (keep_l, self._engine_keep[1], lin) + tuple(self._engine_keep[3:])

    def forward(self, *a, **kw):
        raise RuntimeError("FluxControlNet runs attached to a Flux model: pass controlnet=ControlNetCall(net, cond, scale, mode) to Flux.forward / Flux.denoise")

    denoise = forward

    def load_lora(self, *a, **kw):
        raise NotImplementedError("fluxmi: LoRA on a ControlNet is not supported")

    # ---- the attachment, called by Flux under ITS lock ----------------------------------------------------------------------------------
    def _attach(self, main_engine, cond: Tensor, mode: Optional[int], scale: float):
        """after Flux._prepare: attach this net to the main engine's prepared shape for the call that follows"""
        self._ensure_engine(cond.device)
        trial = self._trial_counter()
        _lib.call("fluxmi_engine_attach_controlnet", main_engine, self._engine, ops._p(cond), cond.shape[0], -1 if mode is None else int(mode),
                  float(scale), trial if trial is not None else 0, ops._stream())

    def _detach(self, main_engine):
        """behind the call: read the net's own calibration counter back, detach"""
        if self._trial_counter() is not None:
            t = C.c_int(0)
            _lib.call("fluxmi_controlnet_trial", self._engine, C.byref(t))
            self._advance_calibration(t.value)
        _lib.call("fluxmi_engine_attach_controlnet", main_engine, None, None, 0, -1, 1.0, 0, ops._stream())

    # ---- loading ------------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, config, sd: Dict[str, Tensor], diffusers_names: Optional[bool] = None) -> "FluxControlNet":
        """A net for the main model of `config` from a diffusers-format (converted here) or already BFL-named state dict; the geometry is read
        off the keys.  bf16 nn.Linear everywhere: quantise with float8_quantize.quantize_flow_transformer_and_dispatch_float8 like Flux."""
        if diffusers_names is None:
            diffusers_names = any(k.startswith(("transformer_blocks.", "x_embedder.")) for k in sd)
        if any(k.startswith("input_hint_block") for k in sd):
            inspect_diffusers_controlnet(sd)  # raises, by name
        if diffusers_names:
            sd = convert_diffusers_controlnet_checkpoint(sd)
        count = lambda pat: len({int(m.group(1)) for k in sd for m in [re.match(pat, k)] if m})
        nd, ns = count(r"controlnet_blocks\.(\d+)\.weight$"), count(r"controlnet_single_blocks\.(\d+)\.weight$")
        mode = sd.get("controlnet_mode_embedder.weight")
        w = sd["controlnet_x_embedder.weight"]
        p = config.params
        if int(w.shape[0]) != p.hidden_size or int(w.shape[1]) != p.in_channels:
            raise ValueError(f"fluxmi: the ControlNet has hidden {w.shape[0]} / in_channels {w.shape[1]}, the main model {p.hidden_size} / {p.in_channels}")
        with torch.device("meta"):
            net = cls(config, nd, ns, 0 if mode is None else int(mode.shape[0]), guidance_embed="guidance_in.in_layer.weight" in sd)
        missing, unexpected = net.load_state_dict(sd, strict=False, assign=True)
        if missing or unexpected:
            raise ValueError(f"fluxmi: ControlNet state dict does not fit: missing {missing[:4]}, unexpected {unexpected[:4]}")
        net.type(torch.bfloat16)
        net.requires_grad_(False)
        return net
