"""Flux flow transformer on MI355X: the module tree of the reference (modules/flux_model.py of
aredden/flux-fp8-api) as a thin parameter container over the native fluxmi engine.

Kept from the reference (so that float8_quantize / lora_loading / pipeline code that WALKS the tree by
name keeps working): class names, constructor arguments, attribute names
(double_blocks[i].img_mod.lin, .img_attn.qkv/.norm.query_norm.scale/.proj, .img_mlp[0|2], ...,
single_blocks[i].linear1/.linear2/.norm/.modulation.lin, final_layer.linear/.adaLN_modulation[1],
img_in, txt_in, time_in, vector_in, guidance_in, pe_embedder), the BFL state-dict key layout,
`Flux.forward(img, img_ids, txt, txt_ids, timesteps, y, guidance)` and the LoRA bookkeeping methods.

Different by design: the modules hold weights only.  `Flux.forward` hands raw device pointers to the C++
engine (csrc/engine.hip, csrc/engine_denoise.hip), which runs the whole step on hand-written gfx950 kernels -- fused and
hipGraph-captured once every F8Linear input scale is frozen, unfused (reference op order) while the
12-trial calibration of float8_quantize.py:220-246 is still running.
"""
from __future__ import annotations

import ctypes as C
import math
import threading
from collections import namedtuple
from typing import TYPE_CHECKING, List, Optional

import torch
from pydantic import BaseModel, Field
from torch import Tensor, nn

from fluxmi import GenerationCancelled, _lib, ops, solvers

if TYPE_CHECKING:
    from util import ModelSpec


# Progress, previews and cancellation of one Flux.denoise call (include/fluxmi.h, fluxmi_engine_set_preview).  proj: the 51 floats of
# ops.preview_proj (None with every = 0); grid: (h, w) tokens of the stepped rows; every: 0 = progress and cancellation only, k > 0 = a preview
# at every evaluation g with g % k == 0; eval_offset / n_evaluations: this call's first evaluation within the request and the request's
# total; callback(evaluation, n_evaluations, rgb) with rgb a uint8 numpy array [images, 2 h, 2 w, 3] or None -- returning False cancels.
PreviewCall = namedtuple("PreviewCall", ["proj", "grid", "every", "eval_offset", "n_evaluations", "callback"])


class FluxParams(BaseModel):  # reference flux_model.py:24-36
    in_channels: int
    vec_in_dim: int
    context_in_dim: int
    hidden_size: int
    mlp_ratio: float
    num_heads: int
    depth: int
    depth_single_blocks: int
    axes_dim: list[int]
    theta: int
    qkv_bias: bool
    guidance_embed: bool
    # BFL's name: the channels the model predicts.  None = in_channels (every text-to-image model).  FLUX.1 Fill [dev] (384 -> 64) and
    # Depth / Canny [dev] (128 -> 64) feed step-invariant conditioning channels behind the 64 noisy ones through img_in.  Not part of
    # model_dump(): the oracle's FluxParams dataclass has no such field.
    out_channels: Optional[int] = Field(default=None, exclude=True)


ModulationOut = namedtuple("ModulationOut", ["shift", "scale", "gate"])


def _f8():
    from float8_quantize import F8Linear

    return F8Linear


def _lin(i, o, bias=True, f8=False):
    return _f8()(in_features=i, out_features=o, bias=bias) if f8 else nn.Linear(i, o, bias=bias)


def timestep_embedding(t: Tensor, dim, max_period=10000, time_factor: float = 1000.0):
    """reference flux_model.py:95-116 (device kernel; `t` is rounded through its own dtype like the reference)."""
    freqs = ops.timestep_freqs_host(dim // 2, max_period).to(t.device)
    return ops.timestep_embedding(t.to(torch.bfloat16), freqs, time_factor)


class EmbedND(nn.Module):  # reference flux_model.py:68-92
    def __init__(self, dim: int, theta: int, axes_dim: list[int], dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        self.dim, self.theta, self.axes_dim, self.dtype = dim, theta, axes_dim, dtype

    def forward(self, ids: Tensor) -> Tensor:
        """Returns the reference layout [B,1,L,dim/2,2,2] = [[cos,-sin],[sin,cos]] built from the device table."""
        pe = ops.rope_table(ids.to(torch.bfloat16), self.axes_dim, self.theta)  # [B,L,P,2]
        c, s = pe[..., 0], pe[..., 1]
        return torch.stack((c, -s, s, c), dim=-1).reshape(*c.shape, 2, 2).unsqueeze(1).to(self.dtype)


class MLPEmbedder(nn.Module):  # reference flux_model.py:119-155
    def __init__(self, in_dim: int, hidden_dim: int, prequantized: bool = False, quantized=False):
        super().__init__()
        self.in_layer = _lin(in_dim, hidden_dim, f8=prequantized and quantized)
        self.silu = nn.SiLU()
        self.out_layer = _lin(hidden_dim, hidden_dim, f8=prequantized and quantized)


class RMSNorm(nn.Module):  # reference flux_model.py:158-164
    def __init__(self, dim: int):
        super().__init__()
        self.scale = nn.Parameter(torch.ones(dim), requires_grad=False)


class QKNorm(nn.Module):  # reference flux_model.py:167-176
    def __init__(self, dim: int):
        super().__init__()
        self.query_norm = RMSNorm(dim)
        self.key_norm = RMSNorm(dim)


class SelfAttention(nn.Module):  # reference flux_model.py:179-227
    def __init__(self, dim: int, num_heads: int = 8, qkv_bias: bool = False, prequantized: bool = False):
        super().__init__()
        self.num_heads = num_heads
        self.qkv = _lin(dim, dim * 3, bias=qkv_bias, f8=prequantized)
        self.norm = QKNorm(dim // num_heads)
        self.proj = _lin(dim, dim, f8=prequantized)


class Modulation(nn.Module):  # reference flux_model.py:233-257
    def __init__(self, dim: int, double: bool, quantized_modulation: bool = False):
        super().__init__()
        self.is_double = double
        self.multiplier = 6 if double else 3
        self.lin = _lin(dim, self.multiplier * dim, f8=quantized_modulation)
        self.act = nn.SiLU()


class DoubleStreamBlock(nn.Module):  # reference flux_model.py:260-400
    def __init__(self, hidden_size: int, num_heads: int, mlp_ratio: float, qkv_bias: bool = False,
                 dtype: torch.dtype = torch.float16, quantized_modulation: bool = False, prequantized: bool = False):
        super().__init__()
        self.dtype, self.num_heads, self.hidden_size = dtype, num_heads, hidden_size
        mlp_hidden_dim = int(hidden_size * mlp_ratio)
        for s in ("img", "txt"):
            setattr(self, f"{s}_mod", Modulation(hidden_size, double=True, quantized_modulation=quantized_modulation))
            setattr(self, f"{s}_norm1", nn.LayerNorm(hidden_size, elementwise_affine=False, eps=1e-6))
            setattr(self, f"{s}_attn", SelfAttention(dim=hidden_size, num_heads=num_heads, qkv_bias=qkv_bias, prequantized=prequantized))
            setattr(self, f"{s}_norm2", nn.LayerNorm(hidden_size, elementwise_affine=False, eps=1e-6))
            setattr(self, f"{s}_mlp", nn.Sequential(_lin(hidden_size, mlp_hidden_dim, f8=prequantized), nn.GELU(approximate="tanh"),
                                                    _lin(mlp_hidden_dim, hidden_size, f8=prequantized)))


class SingleStreamBlock(nn.Module):  # reference flux_model.py:403-485
    def __init__(self, hidden_size: int, num_heads: int, mlp_ratio: float = 4.0, qk_scale: float | None = None,
                 dtype: torch.dtype = torch.float16, quantized_modulation: bool = False, prequantized: bool = False):
        super().__init__()
        self.dtype, self.hidden_dim, self.hidden_size, self.num_heads = dtype, hidden_size, hidden_size, num_heads
        self.mlp_hidden_dim = int(hidden_size * mlp_ratio)
        self.linear1 = _lin(hidden_size, hidden_size * 3 + self.mlp_hidden_dim, f8=prequantized)
        self.linear2 = _lin(hidden_size + self.mlp_hidden_dim, hidden_size, f8=prequantized)
        self.norm = QKNorm(hidden_size // num_heads)
        self.pre_norm = nn.LayerNorm(hidden_size, elementwise_affine=False, eps=1e-6)
        self.mlp_act = nn.GELU(approximate="tanh")
        self.modulation = Modulation(hidden_size, double=False, quantized_modulation=quantized_modulation and prequantized)


class LastLayer(nn.Module):  # reference flux_model.py:488-503
    def __init__(self, hidden_size: int, patch_size: int, out_channels: int):
        super().__init__()
        self.norm_final = nn.LayerNorm(hidden_size, elementwise_affine=False, eps=1e-6)
        self.linear = nn.Linear(hidden_size, patch_size * patch_size * out_channels, bias=True)
        self.adaLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(hidden_size, 2 * hidden_size, bias=True))


class Flux(nn.Module):
    """Transformer model for flow matching on sequences (reference flux_model.py:506-734)."""

    MAX_ENGINE_BATCH = 32  # samples per engine pass (csrc/engine_state.h FLUXMI_ENGINE_MAX_BATCH)

    def __init__(self, config: "ModelSpec", dtype: torch.dtype = torch.float16):
        super().__init__()
        self.dtype = dtype
        self.params = p = config.params
        self.in_channels = p.in_channels
        self.out_channels = p.in_channels if p.out_channels is None else p.out_channels
        if not 0 < self.out_channels <= self.in_channels:
            raise ValueError(f"out_channels {self.out_channels} must be in 1..in_channels ({self.in_channels})")
        self.loras: List = []
        preq = config.prequantized_flow
        q_emb = config.quantize_flow_embedder_layers and preq
        q_mod = config.quantize_modulation and preq
        if p.hidden_size % p.num_heads != 0:
            raise ValueError(f"Hidden size {p.hidden_size} must be divisible by num_heads {p.num_heads}")
        pe_dim = p.hidden_size // p.num_heads
        if sum(p.axes_dim) != pe_dim:
            raise ValueError(f"Got {p.axes_dim} but expected positional dim {pe_dim}")
        self.hidden_size, self.num_heads = p.hidden_size, p.num_heads
        self.pe_embedder = EmbedND(dim=pe_dim, theta=p.theta, axes_dim=p.axes_dim, dtype=self.dtype)
        self.img_in = _lin(self.in_channels, self.hidden_size, f8=q_emb)
        self.time_in = MLPEmbedder(256, self.hidden_size, prequantized=preq, quantized=q_emb)
        self.vector_in = MLPEmbedder(p.vec_in_dim, self.hidden_size, prequantized=preq, quantized=q_emb)
        self.guidance_in = MLPEmbedder(256, self.hidden_size, prequantized=preq, quantized=q_emb) if p.guidance_embed else nn.Identity()
        self.txt_in = _lin(p.context_in_dim, self.hidden_size, f8=q_emb)
        self.double_blocks = nn.ModuleList([
            DoubleStreamBlock(self.hidden_size, self.num_heads, mlp_ratio=p.mlp_ratio, qkv_bias=p.qkv_bias, dtype=self.dtype,
                              quantized_modulation=q_mod, prequantized=preq) for _ in range(p.depth)])
        self.single_blocks = nn.ModuleList([
            SingleStreamBlock(self.hidden_size, self.num_heads, mlp_ratio=p.mlp_ratio, dtype=self.dtype,
                              quantized_modulation=q_mod, prequantized=preq) for _ in range(p.depth_single_blocks)])
        self.final_layer = LastLayer(self.hidden_size, 1, self.out_channels)
        self.requires_grad_(False)
        self._engine = None
        self._engine_keep = None
        self._engine_device = None
        self._lock = threading.Lock()  # the C handle is not re-entrant (the reference's api.py calls from a threadpool)
        self._prep_key = None
        self._amax_xchg = None  # (device array, ctypes callback) of the batch-sharded calibration exchange, see enable_amax_exchange

    # ---- engine plumbing ---------------------------------------------------------------------------------
    def linear_modules(self) -> List[nn.Module]:
        """Linear layers in the canonical order of include/fluxmi.h."""
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
        mods += [self.final_layer.adaLN_modulation[1], self.final_layer.linear]
        return mods

    def f8_modules(self):
        F8 = _f8()
        return [m for m in self.linear_modules() if isinstance(m, F8)]

    def _invalidate_engine(self):
        with self._lock:
            if self._engine is not None:
                _lib.call("fluxmi_engine_destroy", self._engine)
            self._engine, self._engine_keep, self._prep_key, self._engine_device = None, None, None, None

    def __del__(self):
        try:
            if getattr(self, "_engine", None) is not None:
                _lib.lib.fluxmi_engine_destroy(self._engine)
        except Exception:
            pass

    def _linear_table(self, device):
        F8 = _f8()
        mods = self.linear_modules()
        arr = (_lib.Linear * len(mods))()
        keep = []
        for i, m in enumerate(mods):
            L = arr[i]
            if isinstance(m, F8):
                if not m.weight_initialized:
                    m.to(device)
                    m.quantize_weight()
                m._ensure_state(device)
                if m.float8_data.device != device:
                    m.to(device)
                L.weight, L.kind = m.float8_data.data_ptr(), 1
                L.w_scale_recip, L.in_scale = m.scale_reciprocal.data_ptr(), m.input_scale.data_ptr()
                L.in_scale_recip, L.amax_trials = m.input_scale_reciprocal.data_ptr(), m.input_amax_trials.data_ptr()
                L.in_fmt = ops.fmt_of(m.input_float8_dtype)
                L.N, L.K = m.out_features, m.in_features
                keep += [m.float8_data, m.scale_reciprocal, m.input_scale, m.input_scale_reciprocal, m.input_amax_trials]
            else:
                if m.weight.device != device or m.weight.dtype != torch.bfloat16:
                    m.to(device=device, dtype=torch.bfloat16)
                w = m.weight.data.contiguous()
                L.weight, L.kind, L.in_fmt = w.data_ptr(), 0, _lib.E5M2
                L.N, L.K = w.shape
                keep.append(w)
            b = m.bias
            if b is not None:
                bb = b.data.to(device=device, dtype=torch.bfloat16).contiguous()
                L.bias = bb.data_ptr()
                keep.append(bb)
        return arr, keep

    def _norm_table(self, device):
        ts = []
        for b in self.double_blocks:
            ts += [b.img_attn.norm.query_norm.scale, b.img_attn.norm.key_norm.scale, b.txt_attn.norm.query_norm.scale, b.txt_attn.norm.key_norm.scale]
        for b in self.single_blocks:
            ts += [b.norm.query_norm.scale, b.norm.key_norm.scale]
        keep = [t.data.to(device=device, dtype=torch.bfloat16).contiguous() for t in ts]
        arr = (C.c_void_p * len(keep))(*[k.data_ptr() for k in keep])
        return arr, keep

    def _ensure_engine(self, device):
        if self._engine is not None:
            return
        if device.type != "cuda":
            raise RuntimeError("Flux (fluxmi): the model must run on a GPU; there is no CPU path")
        p = self.params
        if p.hidden_size // p.num_heads != 128:
            raise ValueError("fluxmi supports head_dim 128 (every FLUX.1 variant); got %d" % (p.hidden_size // p.num_heads))
        d = _lib.ModelDesc()
        d.hidden, d.heads, d.mlp_hidden = p.hidden_size, p.num_heads, int(p.hidden_size * p.mlp_ratio)
        d.depth, d.depth_single, d.in_channels = p.depth, p.depth_single_blocks, p.in_channels
        d.vec_in, d.ctx_in, d.guidance_embed = p.vec_in_dim, p.context_in_dim, int(p.guidance_embed)
        d.axes_dim = (C.c_int * 3)(*p.axes_dim)
        d.theta = p.theta
        f8 = self.f8_modules()
        d.num_trials = f8[0].num_scale_trials if f8 else 12
        lin, keep_l = self._linear_table(device)
        nrm, keep_n = self._norm_table(device)
        h = C.c_void_p()
        _lib.call("fluxmi_engine_create", C.byref(d), lin, len(lin), nrm, len(nrm), C.byref(h))
        om, ax = ops.rope_tables_host(p.axes_dim, p.theta)
        fr = ops.timestep_freqs_host(128)
        _lib.call("fluxmi_engine_set_tables", h, fr.numpy().ctypes.data_as(C.POINTER(C.c_float)),
                  om.numpy().ctypes.data_as(C.POINTER(C.c_float)), ax.numpy().ctypes.data_as(C.POINTER(C.c_int)))
        self._engine, self._engine_keep, self._prep_key, self._engine_device = h, (keep_l, keep_n, lin, nrm), None, device
        if self._amax_xchg is not None:
            self._install_amax_exchange()

    def rebind_weights(self):
        """Call after weight surgery (LoRA fuse, set_weight_tensor) so the engine sees the new pointers."""
        if self._engine is None:
            return
        dev = self._engine_device  # the device the engine was created on (not necessarily torch's current device)
        lin, keep_l = self._linear_table(dev)
        with self._lock:
            _lib.call("fluxmi_engine_rebind", self._engine, lin, len(lin))
            self._engine_keep = (keep_l, self._engine_keep[1], lin, self._engine_keep[3])

    def _prepare(self, img, img_ids, txt_ids, txt, Lc: int = 0):
        """`img` / `img_ids` hold the whole image stream; with a Kontext reference its last `Lc` rows of each sample are the reference tokens.
        The batch is that of the ids and `txt` (a guided request: twice `img`'s, the negative branches behind the prompt branches)."""
        B, L_img = txt.shape[0], img.shape[1]
        Lt = txt.shape[1]
        # cheap (two small copies + one table kernel; the workspace is only re-allocated when the shape changes)
        ii = img_ids.to(torch.bfloat16).contiguous()
        ti = txt_ids.to(torch.bfloat16).contiguous()
        if Lc:
            _lib.call("fluxmi_engine_prepare_cond", self._engine, B, L_img - Lc, Lc, Lt, ops._p(ii), ops._p(ti), ops._stream())
        else:
            _lib.call("fluxmi_engine_prepare", self._engine, B, L_img, Lt, ops._p(ii), ops._p(ti), ops._stream())

    def _set_attn_groups(self, attn_groups, B: int, L: int, device):
        """after _prepare, under the lock: the token-group attention mask of this call (int32 [B, L] descriptors; fluxmi.ops.attn_descriptors,
        flux_pipeline.build_region_groups), or None = dense.  The engine copies the table and checks self-admission."""
        if attn_groups is None:
            _lib.call("fluxmi_engine_set_attn_groups", self._engine, None, ops._stream())
            return
        g = attn_groups
        if g.dtype not in (torch.int32, torch.uint32) or g.ndim != 2 or g.shape[0] not in (1, B) or g.shape[1] != L:
            raise ValueError(f"attn_groups {g.dtype} {tuple(g.shape)}: expected int32 [1 or {B}, {L}] (one descriptor per token of the joint "
                             f"sequence: text rows, image rows, reference rows)")
        g = g.to(device).expand(B, L).contiguous()
        _lib.call("fluxmi_engine_set_attn_groups", self._engine, ops._p(g), ops._stream())

    def _check_inpaint(self, img, x0, noise, mask, thresholds, n_steps: int):
        """the masked-latent inpainting arguments of a denoise call, validated before any device work -> None (no mask) or (x0, noise, mask
        expanded over the batch, thresholds as a list or None)"""
        given = [t is not None for t in (x0, noise, mask)]
        if not any(given):
            if thresholds is not None:
                raise ValueError("inpaint_thresholds without inpaint_x0 / inpaint_noise / inpaint_mask")
            return None
        if not all(given):
            raise ValueError("inpaint_x0, inpaint_noise and inpaint_mask go together (all three or none)")
        want = (img.shape[0], img.shape[1], self.out_channels)
        for name, t in (("inpaint_x0", x0), ("inpaint_noise", noise)):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != want:
                raise ValueError(f"{name} {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}: expected a tensor {want} (the "
                                 f"stepped channels of img's noisy tokens)")
        if not isinstance(mask, torch.Tensor) or mask.ndim != 3 or mask.shape[0] not in (1, want[0]) or tuple(mask.shape[1:]) != want[1:]:
            raise ValueError(f"inpaint_mask {tuple(mask.shape) if isinstance(mask, torch.Tensor) else type(mask).__name__}: expected a tensor "
                             f"[1 or {want[0]}, {want[1]}, {want[2]}]")
        if thresholds is not None:
            thresholds = [float(t) for t in thresholds]
            if len(thresholds) != n_steps or any(math.isnan(t) for t in thresholds):
                raise ValueError(f"inpaint_thresholds: {len(thresholds)} values for {n_steps} steps (one per step of this call, none NaN)")
        return x0, noise, mask.expand(want[0], -1, -1), thresholds

    def _set_inpaint(self, inpaint, device):
        """after _prepare, under the lock: the masked-latent inpainting state of this call (the engine copies the tensors), or None = off.  Set
        on every call, so nothing is left over from an earlier request."""
        if inpaint is None:
            _lib.call("fluxmi_engine_set_inpaint", self._engine, None, None, None, 0, None, 0, ops._stream())
            return
        x0, noise, mask, thr = inpaint
        x0, noise, mask = (t.to(device=device, dtype=torch.bfloat16).contiguous() for t in (x0, noise, mask))
        table = (C.c_double * len(thr))(*thr) if thr is not None else None
        if thr is not None and not thr:
            table = (C.c_double * 1)()  # a non-NULL table of zero entries: a differential call of zero steps
        _lib.call("fluxmi_engine_set_inpaint", self._engine, ops._p(x0), ops._p(noise), ops._p(mask), x0.shape[0], table,
                  len(thr) if thr is not None else 0, ops._stream())

    def _set_solver(self, solver):
        """after _prepare, under the lock: the solver program of this call (fluxmi.solvers.SolverProgram), or None = off"""
        if solver is None:
            _lib.call("fluxmi_engine_set_solver", self._engine, None, None, 0)
            return
        n = len(solver.coef)
        coef = (C.c_double * max(1, 8 * n))(*[float(v) for row in solver.coef for v in row])
        ctl = (C.c_int * max(1, 4 * n))(*[int(v) for row in solver.ctl for v in row])
        _lib.call("fluxmi_engine_set_solver", self._engine, coef, ctl, n)

    def _set_solver_noise(self, solver_noise):
        """after _set_solver, under the lock: the per-image noise ids and evaluation offset of a stochastic program (_check_solver_noise)"""
        if solver_noise is None:
            return
        ids, off = solver_noise
        flat = (C.c_uint32 * (4 * len(ids)))(*[w for row in ids for w in row])
        _lib.call("fluxmi_engine_set_solver_noise", self._engine, flat, len(ids), off)

    GUIDANCE_SHAPING_KEYS = ("mode", "rescale", "eta", "norm_threshold", "momentum", "zero_init_steps", "step_offset")

    @classmethod
    def _check_guidance_shaping(cls, shaping, guided, cfg_scale):
        """`guidance_shaping` of denoise -> (the 8 floats of fluxmi_guidance_combine, step_offset), or None"""
        if shaping is None:
            return None
        if not guided:
            raise ValueError("guidance_shaping needs a negative prompt (neg_txt / neg_y): it shapes the true-CFG combination of the two branches")
        if not isinstance(shaping, dict) or set(shaping) - set(cls.GUIDANCE_SHAPING_KEYS):
            raise ValueError(f"guidance_shaping: expected a dict with keys out of {cls.GUIDANCE_SHAPING_KEYS}, got {shaping!r}")
        mode = shaping.get("mode", "cfg")
        if mode not in ops.GUIDANCE_MODES:
            raise ValueError(f"guidance_shaping: unknown mode {mode!r} (one of {sorted(ops.GUIDANCE_MODES)})")
        phi, eta, rho, mu = (float(shaping.get(k, d)) for k, d in (("rescale", 0.0), ("eta", 1.0), ("norm_threshold", 0.0), ("momentum", 0.0)))
        zi, off = int(shaping.get("zero_init_steps", 0)), int(shaping.get("step_offset", 0))
        if not all(math.isfinite(v) for v in (phi, eta, rho, mu, float(cfg_scale))):
            raise ValueError("guidance_shaping: every value (and cfg_scale) must be finite")
        if not 0.0 <= phi <= 1.0:
            raise ValueError(f"guidance_shaping: rescale {phi} outside [0, 1]")
        if rho < 0.0 or zi < 0 or off < 0:
            raise ValueError(f"guidance_shaping: norm_threshold {rho}, zero_init_steps {zi} and step_offset {off} must be >= 0")
        return ops.guidance_params(cfg_scale, mode, phi, eta, rho, mu, zi), off

    @staticmethod
    def _check_preview(preview):
        if preview is None:
            return None
        if not callable(preview.callback):
            raise ValueError("preview: callback must be callable")
        every, off, n = int(preview.every), int(preview.eval_offset), int(preview.n_evaluations)
        if every < 0 or off < 0 or n < 0:
            raise ValueError(f"preview: every {every}, eval_offset {off} and n_evaluations {n} must be >= 0")
        proj = None
        if every > 0:
            proj = [float(v) for v in preview.proj]
            if len(proj) != 51 or not all(math.isfinite(v) for v in proj):
                raise ValueError("preview: proj holds 51 finite floats (ops.preview_proj)")
            if len(preview.grid) != 2:
                raise ValueError("preview: grid = (h, w) tokens")
        return PreviewCall(proj, tuple(int(v) for v in preview.grid) if every > 0 else (0, 0), every, off, n, preview.callback)

    def _set_preview(self, preview):
        """after _prepare, under the lock: the step hook of this call (_check_preview) -> the state that keeps the ctypes callback alive and
        carries an exception out of it (ctypes would swallow it), or None"""
        if preview is None:
            return None
        import numpy as np

        state = {"error": None, "cb": None}

        def hook(user, evaluation, n_evaluations, rgb, images, height, width):
            try:
                arr = None
                if rgb:
                    buf = (C.c_ubyte * (images * height * width * 3)).from_address(rgb)
                    arr = np.frombuffer(buf, dtype=np.uint8).reshape(images, height, width, 3).copy()  # the pinned buffer is the engine's
                return 1 if preview.callback(evaluation, n_evaluations, arr) is False else 0
            except BaseException as e:  # an exception must not cross the C ABI: cancel, re-raise behind the engine call
                state["error"] = e
                return 1

        state["cb"] = _lib.STEP_HOOK(hook)
        proj = (C.c_float * 51)(*preview.proj) if preview.proj is not None else None
        _lib.call("fluxmi_engine_set_preview", self._engine, proj, preview.grid[0], preview.grid[1], preview.every, preview.eval_offset,
                  preview.n_evaluations, state["cb"], None)
        return state

    def preview_stats(self):
        """(graph captures of the engine since it was created, evaluations the last denoise call launched): read-only, for tests"""
        if self._engine is None:
            return 0, 0
        with self._lock:
            cap, ran = C.c_longlong(0), C.c_int(0)
            _lib.call("fluxmi_engine_preview_stats", self._engine, C.byref(cap), C.byref(ran))
        return cap.value, ran.value

    def _set_guidance(self, shaping):
        """after _prepare, under the lock: the shaping state of this call (_check_guidance_shaping), or None = off.  Every set call with a
        state starts APG's running difference at 0."""
        if shaping is None:
            _lib.call("fluxmi_engine_set_guidance", self._engine, None, 0)
            return
        _lib.call("fluxmi_engine_set_guidance", self._engine, (C.c_float * 8)(*shaping[0]), shaping[1])

    @staticmethod
    def _check_solver_noise(solver_noise, solver, B):
        """-> (ids: a list of B 4-tuples of uint32 words, eval_offset) or None"""
        if solver_noise is None:
            if solver is not None and solvers.has_noise(solver):
                raise ValueError("solver: the program draws noise (a non-zero cn) -- pass solver_noise=(ids [B, 4], eval_offset)")
            return None
        if solver is None or not solvers.has_noise(solver):
            raise ValueError("solver_noise needs a solver program that draws noise (a non-zero cn in some row)")
        try:
            ids, off = solver_noise
            ids = ids.tolist() if isinstance(ids, Tensor) else [list(r) for r in ids]
            ids = [tuple(int(w) & 0xffffffff for w in r) for r in ids]  # (an int32 tensor holds the words' bits)
            off = int(off)
        except (TypeError, ValueError):
            raise ValueError("solver_noise: expected (ids [B, 4] uint32 / int tensor or list, eval_offset)") from None
        if len(ids) != B or any(len(r) != 4 for r in ids):
            raise ValueError(f"solver_noise: ids of {len(ids)} images for a batch of {B} (one {{key_lo, key_hi, c2, c3}} per image)")
        if not 0 <= off < 2 ** 31:
            raise ValueError(f"solver_noise: eval_offset {off} outside [0, 2^31)")
        return ids, off

    @staticmethod
    def _with_reference(img, img_ids, img_cond_seq, img_cond_seq_ids):
        """FLUX.1 Kontext: the reference tokens ride behind the noisy tokens of each sample -> (stream, stream ids, Lc).  Both None: unchanged."""
        if img_cond_seq is None and img_cond_seq_ids is None:
            return img, img_ids, 0
        if img_cond_seq is None or img_cond_seq_ids is None:
            raise ValueError("img_cond_seq and img_cond_seq_ids go together")
        if img_cond_seq.ndim != 3 or img_cond_seq.shape[0] != img.shape[0] or img_cond_seq.shape[2] != img.shape[2]:
            raise ValueError(f"img_cond_seq {tuple(img_cond_seq.shape)} does not match img {tuple(img.shape)}")
        if tuple(img_cond_seq_ids.shape) != (img_cond_seq.shape[0], img_cond_seq.shape[1], 3):
            raise ValueError(f"img_cond_seq_ids {tuple(img_cond_seq_ids.shape)} != {(img_cond_seq.shape[0], img_cond_seq.shape[1], 3)}")
        Lc = img_cond_seq.shape[1]
        if Lc == 0:
            return img, img_ids, 0
        img = torch.cat((img.to(torch.bfloat16), img_cond_seq.to(device=img.device, dtype=torch.bfloat16)), 1)
        img_ids = torch.cat((img_ids, img_cond_seq_ids.to(device=img_ids.device, dtype=img_ids.dtype)), 1)
        return img, img_ids, Lc

    def _with_channels(self, img, img_cond, img_cond_seq):
        """FLUX.1 Fill / Depth / Canny: the conditioning channels ride behind the noisy channels of every token -> [B, Li, in_channels].
        `img_cond` [B, Li, in_channels - out_channels] is required exactly when the two differ; no released model takes it together with
        a Kontext `img_cond_seq` (the engine refuses the combination).  Checked before any device work."""
        extra = self.in_channels - self.out_channels
        if img_cond is None:
            if extra:
                raise ValueError(f"this model takes {extra} conditioning channels per token (in_channels {self.in_channels}, out_channels "
                                 f"{self.out_channels}): pass img_cond [B, Li, {extra}]")
            return img
        if not extra:
            raise ValueError(f"img_cond given, but this model has no conditioning channels (in_channels == out_channels == {self.in_channels})")
        if img_cond_seq is not None:
            raise ValueError("img_cond (channel conditioning) and img_cond_seq (a Kontext reference) cannot be combined")
        if img.shape[2] != self.out_channels:
            raise ValueError(f"img {tuple(img.shape)}: expected {self.out_channels} noisy channels per token")
        if img_cond.ndim != 3 or tuple(img_cond.shape) != (img.shape[0], img.shape[1], extra):
            raise ValueError(f"img_cond {tuple(img_cond.shape)} != {(img.shape[0], img.shape[1], extra)}")
        return torch.cat((img.to(torch.bfloat16), img_cond.to(device=img.device, dtype=torch.bfloat16)), 2)

    def _check_controlnet(self, controlnet, img, B_cond: int, kontext: bool, attn_groups, cache_threshold: float = 0.0):
        """the `controlnet=` argument (modules.controlnet.ControlNetCall) validated before any device work -> None or (net, cond, mode, scale)"""
        if controlnet is None:
            return None
        net, cond, scale, mode = controlnet.net, controlnet.cond, float(controlnet.scale), controlnet.mode
        if self.in_channels != self.out_channels:
            raise ValueError("controlnet: FLUX.1 Fill / Depth / Canny [dev] models (in_channels != out_channels) take no ControlNet")
        if kontext:
            raise ValueError("controlnet: a Kontext reference (img_cond_seq) does not combine with a ControlNet")
        if attn_groups is not None:
            raise ValueError("controlnet: regional prompts (attn_groups) do not combine with a ControlNet")
        if cache_threshold > 0.0:
            raise ValueError("controlnet: step caching (cache_threshold > 0) does not combine with a ControlNet")
        if net.hidden_size != self.hidden_size or net.num_heads != self.num_heads or net.in_channels != self.in_channels:
            raise ValueError(f"controlnet: the net's hidden / heads / in_channels ({net.hidden_size} / {net.num_heads} / {net.in_channels}) differ "
                             f"from the main model's ({self.hidden_size} / {self.num_heads} / {self.in_channels})")
        if net.params.guidance_embed and not self.params.guidance_embed:
            raise ValueError("controlnet: the net has a guidance embedder, the main model has none")
        if net.is_union:
            if mode is None or not 0 <= int(mode) < net.num_mode:
                raise ValueError(f"controlnet: a Union net needs control_mode in 0..{net.num_mode - 1} (got {mode})")
        elif mode is not None:
            raise ValueError("controlnet: control_mode given to a net without a mode embedding")
        if not math.isfinite(scale):
            raise ValueError(f"controlnet: conditioning scale {scale} is not finite")
        want = (B_cond, img.shape[1], self.in_channels)
        if not isinstance(cond, torch.Tensor) or cond.ndim != 3 or cond.shape[0] not in (1, B_cond) or tuple(cond.shape[1:]) != want[1:]:
            raise ValueError(f"controlnet: cond {tuple(cond.shape) if isinstance(cond, torch.Tensor) else type(cond).__name__}: expected a tensor "
                             f"[1 or {want[0]}, {want[1]}, {want[2]}] (the packed control latent)")
        return net, cond.expand(B_cond, -1, -1), None if mode is None else int(mode), scale

    def _attach_controlnet(self, cn, device):
        """after _prepare, under the lock: attach the call's ControlNet (the engine copies cond), or detach; returns the net to hand to
        _release_controlnet behind the call"""
        if cn is None:
            return None  # nothing is attached between calls (_release_controlnet): a plain call makes the host calls it always made
        net, cond, mode, scale = cn
        net._attach(self._engine, cond.to(device=device, dtype=torch.bfloat16).contiguous(), mode, scale)
        return net

    def _release_controlnet(self, net):
        if net is not None:
            net._detach(self._engine)

    def _check_ip_adapter(self, ip_adapter, B_engine: int, attn_groups, cache_threshold: float = 0.0):
        """the `ip_adapter=` argument (modules.ip_adapter.IPAdapterCall) validated before any device work -> None or (k_ip, v_ip, scales) for
        the B_engine samples of the engine pass (both branches of a guided call): k_ip, v_ip [depth, B_engine, Nk, hidden], scales a
        [B_engine, depth] float32 CPU tensor"""
        if ip_adapter is None:
            return None
        if attn_groups is not None:
            raise ValueError("ip_adapter: regional prompts (attn_groups) do not combine with an IP-Adapter")
        if cache_threshold > 0.0:
            raise ValueError("ip_adapter: step caching (cache_threshold > 0) does not combine with an IP-Adapter")
        k, v = ip_adapter.k_ip, ip_adapter.v_ip
        depth = len(self.double_blocks)
        if not (isinstance(k, torch.Tensor) and isinstance(v, torch.Tensor)) or k.ndim != 4 or k.shape != v.shape or k.shape[0] != depth \
                or k.shape[1] not in (1, B_engine) or k.shape[3] != self.hidden_size:
            raise ValueError(f"ip_adapter: k_ip / v_ip {tuple(getattr(k, 'shape', ()))} / {tuple(getattr(v, 'shape', ()))}: expected two tensors "
                             f"[{depth}, 1 or {B_engine}, Nk, {self.hidden_size}]")
        if not 1 <= k.shape[2] <= 64:
            raise ValueError(f"ip_adapter: Nk = {k.shape[2]} image tokens outside 1..64")
        if self.hidden_size != self.num_heads * 128:
            raise ValueError("ip_adapter: the adapter kernel needs heads of 128")
        from modules.ip_adapter import scale_table

        return k.expand(-1, B_engine, -1, -1), v.expand(-1, B_engine, -1, -1), scale_table(ip_adapter.scale, depth, B_engine)

    def _set_ip_adapter(self, ip, device):
        """after _prepare, under the lock: hand the call's adapter tables to the engine (it copies them), or nothing: no adapter is set
        between calls (_clear_ip_adapter), so a plain call makes the host calls it always made"""
        if ip is None:
            return False
        k, v, sc = ip
        k = k.to(device=device, dtype=torch.bfloat16).contiguous()
        v = v.to(device=device, dtype=torch.bfloat16).contiguous()
        sc = sc.contiguous()
        _lib.call("fluxmi_engine_set_ip_adapter", self._engine, ops._p(k), ops._p(v), int(k.shape[2]), int(k.shape[1]),
                  sc.numpy().ctypes.data_as(C.POINTER(C.c_float)), ops._stream())
        return True

    def _clear_ip_adapter(self, was_set):
        if was_set:
            _lib.call("fluxmi_engine_set_ip_adapter", self._engine, None, None, 0, 0, None, ops._stream())

    # ---- batch-sharded calibration ------------------------------------------------------------------
    def enable_amax_exchange(self, reduce_fn=None):
        """Keep the F8Linear input scales of batch-sharded replicas IDENTICAL to those of the whole batch on one GPU: the reference
        takes amax over the whole batch (float8_quantize.py:227), so during the calibrating steps every layer's running amax is
        MAX-reduced across the ranks before its scale update (fluxmi_engine_set_amax_exchange).  `reduce_fn(tensor)` performs the
        in-place reduction of a small fp32 device tensor on the current stream; default: torch.distributed all_reduce(MAX) over
        RCCL.  Pass reduce_fn=False to uninstall."""
        if reduce_fn is False:
            self._amax_xchg = None
            if self._engine is not None:
                with self._lock:
                    _lib.call("fluxmi_engine_set_amax_exchange", self._engine, None, 0, None, None)
            return
        if reduce_fn is None:
            import torch.distributed as td

            reduce_fn = lambda t: td.all_reduce(t, op=td.ReduceOp.MAX)
        self._amax_xchg = {"fn": reduce_fn, "buf": None, "cb": None, "error": None}
        if self._engine is not None:
            with self._lock:
                self._install_amax_exchange()

    def _install_amax_exchange(self):
        x = self._amax_xchg
        n = len(self.linear_modules())
        x["buf"] = torch.zeros(n, dtype=torch.float32, device=self._engine_device)

        def hook(user, first, count, stream):
            try:  # called by the engine between the amax reduction of layers [first, first+count) and their scale update
                x["fn"](x["buf"][first:first + count])
                return 0
            except Exception as e:  # an exception must not cross the C ABI
                x["error"] = e
                return 1

        x["cb"] = _lib.AMAX_HOOK(hook)
        _lib.call("fluxmi_engine_set_amax_exchange", self._engine, ops._p(x["buf"]), n, x["cb"], None)

    # ---- calibration bookkeeping (mirrors F8Linear.trial_index / input_scale_initialized) -----------------
    def calibration_state(self):
        f8 = self.f8_modules()
        if not f8:
            return None, 0
        return all(m.input_scale_initialized for m in f8), min(m.trial_index for m in f8)

    def _advance_calibration(self, new_trial_index: int):
        for m in self.f8_modules():
            if new_trial_index > m.num_scale_trials:
                m.trial_index, m.input_scale_initialized = m.num_scale_trials, True
            else:
                m.trial_index = new_trial_index

    def _trial_counter(self):
        frozen, t = self.calibration_state()
        if frozen is None:
            return None
        f8 = self.f8_modules()
        return f8[0].num_scale_trials + 1 if frozen else t

    # ---- LoRA bookkeeping (reference flux_model.py:621-670) --------------------------------------------------
    def get_lora(self, identifier: str):
        for lora in self.loras:
            if lora.path == identifier or lora.name == identifier:
                return lora

    def has_lora(self, identifier: str):
        return self.get_lora(identifier) is not None

    def load_lora(self, path: str, scale: float, name: str = None):
        from lora_loading import LoraWeights, apply_lora_to_model, remove_lora_from_module

        if self.has_lora(path):
            lora = self.get_lora(path)
            if lora.scale != scale:
                remove_lora_from_module(self, lora, lora.scale)
                apply_lora_to_model(self, lora, scale)
                lora.scale = scale
        else:
            _, lora = apply_lora_to_model(self, path, scale, return_lora_resolved=True)
            self.loras.append(LoraWeights(lora, path if isinstance(path, str) else (name or "lora"), name, scale))
        self.rebind_weights()

    def unload_lora(self, path_or_identifier: str):
        from lora_loading import remove_lora_from_module

        for idx, lora_ in enumerate(list(self.loras)):
            if lora_.path == path_or_identifier or lora_.name == path_or_identifier:
                remove_lora_from_module(self, lora_.weights, lora_.scale)
                self.loras.pop(idx)
                self.rebind_weights()
                return True
        return False

    # ---- forward / denoise ---------------------------------------------------------------------------------------
    @torch.inference_mode()
    def forward(self, img: Tensor, img_ids: Tensor, txt: Tensor, txt_ids: Tensor, timesteps: Tensor, y: Tensor,
                guidance: Tensor | None = None, mode: Optional[int] = None, img_cond_seq: Tensor | None = None,
                img_cond_seq_ids: Tensor | None = None, img_cond: Tensor | None = None, attn_groups: Tensor | None = None,
                controlnet=None, ip_adapter=None) -> Tensor:
        """One denoise-step evaluation (reference flux_model.py:672-716).  mode=None picks what the reference would do:
        calibrating (unfused) while any F8Linear still has trials to record, fused once frozen.
        FLUX.1 Kontext: `img_cond_seq` [B, Lc, C] / `img_cond_seq_ids` [B, Lc, 3] (flux_pipeline.prepare_kontext_reference) run through every
        block behind the noisy tokens; the prediction covers the `img.shape[1]` noisy tokens only.
        FLUX.1 Fill / Depth / Canny: `img_cond` [B, Li, in_channels - out_channels] (flux_pipeline.prepare_fill_conditioning /
        prepare_control_conditioning) is appended to the channels of every token; the prediction is [B, Li, out_channels].
        `attn_groups`: a token-group attention mask, int32 [1 or B, Lt + Li + Lc] descriptors (include/fluxmi.h, fluxmi_attention_grouped):
        every attention of the forward then runs F.scaled_dot_product_attention(q, k, v, attn_mask=allowed) instead of the dense one.
        `controlnet`: a modules.controlnet.ControlNetCall -- the ControlNet runs first on the same inputs and its per-block residuals, times
        the conditioning scale, are added to the image stream behind the main blocks (diffusers' FluxControlNetModel / FluxTransformer2DModel);
        it calibrates on its own counter.  None = today's call.
        `ip_adapter`: a modules.ip_adapter.IPAdapterCall -- behind every double block the image stream gains ip_scale times the decoupled
        cross-attention of the block's image query over the adapter's image tokens (csrc/ip_attention.hip), before a ControlNet's residual.
        Refused with attn_groups.  None = today's call."""
        if img.ndim != 3 or txt.ndim != 3:
            raise ValueError("Input img and txt tensors must have 3 dimensions.")
        if self.params.guidance_embed and guidance is None:
            raise ValueError("Didn't get guidance strength for guidance distilled model.")
        bf = lambda t: t.to(torch.bfloat16).contiguous()
        Li = img.shape[1]
        cn = self._check_controlnet(controlnet, img, img.shape[0], img_cond_seq is not None or img_cond_seq_ids is not None, attn_groups)
        ip = self._check_ip_adapter(ip_adapter, img.shape[0], attn_groups)
        img = self._with_channels(img, img_cond, img_cond_seq)
        img, img_ids, Lc = self._with_reference(img, img_ids, img_cond_seq, img_cond_seq_ids)
        img, txt, y, timesteps = bf(img), bf(txt), bf(y), bf(timesteps)
        guidance = bf(guidance) if guidance is not None else None
        self._ensure_engine(img.device)
        with self._lock:
            self._prepare(img, img_ids, txt_ids, txt, Lc)
            self._set_attn_groups(attn_groups, img.shape[0], txt.shape[1] + img.shape[1], img.device)
            trial = self._trial_counter()
            if mode is None:
                if trial is None:
                    mode = 2
                elif trial <= self.f8_modules()[0].num_scale_trials:
                    mode = 0
                else:
                    mode = 1 if self._all_block_linears_f8() else 2
            pred = torch.empty(img.shape[0], Li, self.out_channels, dtype=torch.bfloat16, device=img.device)
            net = self._attach_controlnet(cn, img.device)
            try:
                ip_set = self._set_ip_adapter(ip, img.device)
                try:
                    _lib.call("fluxmi_engine_forward", self._engine, ops._p(img), ops._p(txt), ops._p(y), ops._p(timesteps), ops._p(guidance),
                              ops._p(pred), mode, trial if mode == 0 else 0, ops._stream())
                finally:
                    self._clear_ip_adapter(ip_set)
            finally:
                self._release_controlnet(net)
            if mode == 0:
                self._advance_calibration(trial + 1)
        return pred if self.dtype == torch.bfloat16 else pred.to(self.dtype)

    def _all_block_linears_f8(self):
        F8 = _f8()
        for b in self.double_blocks:
            for s in ("img", "txt"):
                a, m = getattr(b, f"{s}_attn"), getattr(b, f"{s}_mlp")
                if not all(isinstance(x, F8) for x in (a.qkv, a.proj, m[0], m[2])):
                    return False
        return all(isinstance(b.linear1, F8) and isinstance(b.linear2, F8) for b in self.single_blocks)

    @torch.inference_mode()
    def denoise(self, img: Tensor, img_ids: Tensor, txt: Tensor, txt_ids: Tensor, y: Tensor, timesteps: List[float],
                guidance: float = 3.5, use_graph: bool = True, img_cond_seq: Tensor | None = None,
                img_cond_seq_ids: Tensor | None = None, img_cond: Tensor | None = None, neg_txt: Tensor | None = None,
                neg_y: Tensor | None = None, cfg_scale: float = 1.0, cache_threshold: float = 0.0, cache_max_hits: int = 0,
                attn_groups: Tensor | None = None, inpaint_x0: Tensor | None = None, inpaint_noise: Tensor | None = None,
                inpaint_mask: Tensor | None = None, inpaint_thresholds=None, controlnet=None, solver=None, solver_noise=None,
                ip_adapter=None, guidance_shaping: dict | None = None, preview: PreviewCall | None = None) -> Tensor:
        """The Euler loop of FluxPipeline.generate (reference flux_pipeline.py:619-651) run natively: calibrating
        steps unfused, every later step one replay of a captured hipGraph.  Returns the final latent tokens.
        FLUX.1 Kontext: with `img_cond_seq` / `img_cond_seq_ids` the reference tokens join every step's forward and are never stepped; the
        return value is the `img.shape[1]` noisy tokens only.
        FLUX.1 Fill / Depth / Canny: `img_cond` [B, Li, in_channels - out_channels] joins every step's forward as further channels of each
        token and is never stepped; the return value is the stepped [B, Li, out_channels] tokens.
        True classifier-free guidance: with `neg_txt` [1 or B, Lt, ctx] / `neg_y` [1 or B, vec] (both or neither; the prompt's Lt) every step
        predicts both branches in ONE forward on 2B samples (prompt branches first, ids and conditioning duplicated) and steps the shared
        latent with `u + cfg_scale * (c - u)` (csrc/update_step.hip, the guided arm of euler_kernel); any `cfg_scale` is taken as given.  At most 16 images
        per pass then, more run as equal passes (frozen scales only); the two branches of an image always share a pass.
        First-block step caching: `cache_threshold` > 0 lets a frozen step whose first double block's residual moved by less than that
        (relative L1, per sample; every sample of the pass must agree) reuse the remaining blocks' residual of the last full step instead of
        running them; at most `cache_max_hits` such steps in a row (0 = no bound).  0 (the default) = off: the call is today's, bit for bit.
        Every call starts with an empty cache; `step_cache_log()` tells what the last call did.
        `attn_groups`: a token-group attention mask for every attention of every step (Flux.forward), int32 [1 or B, Lt + Li + Lc]; a guided
        call takes [2 or 2B, ...]: the tables of the prompt branches, then those of the negative branches.  None = dense, today's call.
        Masked-latent inpainting: `inpaint_x0` (the init image's latent tokens) and `inpaint_noise` (the request's pure noise draw), both
        [B, Li, out_channels], and `inpaint_mask` [1 or B, Li, out_channels] (1 = regenerate, 0 = keep), all three or none.  Every step's
        update -- calibrating, replayed, cached, guided -- is then followed, in the same kernel (csrc/update_step.hip, the BLEND arms of euler_kernel), by
            p = t_next * noise + (1.0 - t_next) * x0;  x' = (1 - m) * p + m * x1
        on bf16 tensors, t_next = timesteps[i + 1]: with a schedule that ends at 0 the kept elements of the result are x0 bit for bit.
        `inpaint_thresholds` (differential diffusion): one float per step of THIS call; step i blends with the binary mask
        float32(m) > float32(thresholds[i]) instead of m.  The caller's tensors are not modified.
        `controlnet`: a modules.controlnet.ControlNetCall (Flux.forward): every step runs the ControlNet, then the main model with the
        residual adds, then the update the request already had -- one captured graph per frozen step once BOTH nets are calibrated; a guided
        request controls both branches.  Refused with a Kontext reference, attn_groups, cache_threshold > 0 and channel-conditioned models.
        `solver`: a fluxmi.solvers.SolverProgram built from `timesteps` (build_program): every update -- calibrating, replayed, guided,
        masked -- is then the table-driven kernel (csrc/update_step.hip, solver_step_kernel) on the program's rows, one engine step per model
        EVALUATION at `solver.times`; `inpaint_thresholds` stays one per user step and is expanded through `solver.step_of_eval`.  Refused
        with cache_threshold > 0: the cache compares consecutive evaluations, and Heun evaluates one time twice.  None = today's call.
        `solver_noise` = (ids, eval_offset) goes with a program that draws noise (fluxmi.solvers.STOCHASTIC_SAMPLERS; a non-zero cn): ids
        [B, 4] uint32 words {key_lo, key_hi, c2, c3} per IMAGE (a tensor or a list; never per branch), eval_offset the index of this call's
        first evaluation within the request.  Evaluation j adds cn * z in the same kernel, z generated there (Philox4x32-10 + Box-Muller) as
        a pure function of (ids[b], j + eval_offset, element): a sample's bits depend on its ids alone, not on its batch or pass.
        `ip_adapter`: a modules.ip_adapter.IPAdapterCall (Flux.forward): every step adds the adapter term behind every double block, in the
        calibrating and the graph-replayed steps alike; K / V and the scales are device data of ONE captured graph.  Its tensors hold 1 or B
        samples, a guided call's 2 or 2B: the prompt branches' tables, then the negative branches'.  Refused with attn_groups and
        cache_threshold > 0.
        `guidance_shaping` (a guided call only): a dict out of {mode: "cfg" | "apg" | "cfg_zero_star", rescale, eta, norm_threshold,
        momentum, zero_init_steps, step_offset}.  Every step then runs two more launches in front of its update (csrc/guidance.hip): per-image
        moments of (c, u, r), and p = alpha c + beta u + gamma r written over both branches' predictions, with `cfg_scale` as s -- CFG
        rescale (`rescale` = phi), adaptive projected guidance (`eta`, `norm_threshold` = rho, `momentum` = mu; the running difference r
        starts at 0 in every call and pass and advances once per model evaluation) and CFG-Zero* (the optimised scale s*; `zero_init_steps`
        = the number of leading model EVALUATIONS of the request whose prediction is replaced by 0, counted from `step_offset` for a call
        that continues a request; Heun and midpoint evaluate twice per step).  The formulas are those of include/fluxmi.h
        (fluxmi_guidance_combine).  The values are device data of one captured graph; shaped versus unshaped is a graph kind.  None =
        today's call, launch for launch.
        `preview`: a PreviewCall.  Its callback is called once per model evaluation, in order, from this thread, behind the GPU's work on
        that evaluation; with `every` > 0 one more launch in front of every update (csrc/preview.hip) projects the denoised estimate
        x - t v to uint8 RGB at latent resolution, and the callback receives it at the evaluations `every` selects.  The host loop then
        stays at most two evaluations ahead of the GPU and the call is synchronous.  Returning False from the callback stops the launches:
        the engine finishes what it launched (cancelling at evaluation k runs min(n, k + 2)), the calibration counters advance by what
        ran, and GenerationCancelled is raised; an exception raised in the callback cancels the same way and is re-raised.  Refused when
        the batch needs more than one engine pass and under an amax exchange (a process group).  None = today's call, launch for launch."""
        n_user = len(timesteps) - 1
        preview = self._check_preview(preview)
        if preview is not None and getattr(self, "_amax_xchg", None) is not None:
            raise ValueError("fluxmi: preview / progress / cancellation are refused under an amax exchange (a process group)")
        if solver is not None:
            if cache_threshold and float(cache_threshold) > 0:
                raise ValueError("fluxmi: a sampler other than euler does not combine with cache_threshold > 0 (the step cache compares "
                                 "consecutive evaluations; a solver may evaluate one time twice)")
            n_eval = len(solver.coef)
            if len(solver.times) != n_eval + 1 or len(solver.ctl) != n_eval or len(solver.step_of_eval) != n_eval:
                raise ValueError(f"solver: {len(solver.times)} times, {len(solver.ctl)} ctl rows and {len(solver.step_of_eval)} step indices for "
                                 f"{n_eval} evaluations")
            if (max(solver.step_of_eval) + 1 if n_eval else 0) != n_user:
                raise ValueError(f"solver: a program of {max(solver.step_of_eval) + 1 if n_eval else 0} steps for {n_user} steps of timesteps "
                                 f"(build it from the same list)")
            ts_f = [float(t) for t in timesteps]
            inside = all(ts_f[i + 1] <= float(solver.times[j]) <= ts_f[i] for j, i in enumerate(solver.step_of_eval))
            if not inside or float(solver.times[-1]) != ts_f[-1]:
                raise ValueError("solver: the program's evaluation times do not lie inside the steps of timesteps (build it from the same list)")
        solver_noise = self._check_solver_noise(solver_noise, solver, img.shape[0])
        shaping = self._check_guidance_shaping(guidance_shaping, neg_txt is not None or neg_y is not None, cfg_scale)
        inpaint = self._check_inpaint(img, inpaint_x0, inpaint_noise, inpaint_mask, inpaint_thresholds, n_user)
        cache_threshold, cache_max_hits = float(cache_threshold), int(cache_max_hits)
        if not (math.isfinite(cache_threshold) and cache_threshold >= 0.0) or cache_max_hits < 0:
            raise ValueError(f"cache_threshold {cache_threshold} must be finite and >= 0 (0 = off), cache_max_hits {cache_max_hits} >= 0 (0 = no bound)")
        bf = lambda t: t.to(torch.bfloat16).contiguous()
        kontext = img_cond_seq is not None or img_cond_seq_ids is not None
        guided = neg_txt is not None or neg_y is not None
        cn = self._check_controlnet(controlnet, img, img.shape[0], kontext, attn_groups, cache_threshold)
        if ip_adapter is not None and guided and ip_adapter.k_ip.ndim == 4 and ip_adapter.k_ip.shape[1] == 2 and img.shape[0] > 1:
            rep = lambda t: t.repeat_interleave(img.shape[0], 1)  # [pos, neg] -> B x pos, B x neg
            sc = ip_adapter.scale
            ip_adapter = type(ip_adapter)(rep(ip_adapter.k_ip), rep(ip_adapter.v_ip),
                                          sc.repeat_interleave(img.shape[0], 0) if isinstance(sc, torch.Tensor) and sc.ndim == 2 else sc)
        ip = self._check_ip_adapter(ip_adapter, img.shape[0] * (2 if guided else 1), attn_groups, cache_threshold)
        if guided:
            if neg_txt is None or neg_y is None:
                raise ValueError("neg_txt and neg_y go together (the negative prompt's T5 sequence and pooled CLIP vector)")
            B = img.shape[0]
            if neg_txt.ndim != 3 or neg_txt.shape[0] not in (1, B) or tuple(neg_txt.shape[1:]) != tuple(txt.shape[1:]):
                raise ValueError(f"neg_txt {tuple(neg_txt.shape)}: expected [1 or {B}, {txt.shape[1]}, {txt.shape[2]}] (the prompt's sequence length: both "
                                 f"branches run in one batch)")
            if neg_y.ndim != 2 or neg_y.shape[0] not in (1, B) or neg_y.shape[1] != y.shape[1]:
                raise ValueError(f"neg_y {tuple(neg_y.shape)}: expected [1 or {B}, {y.shape[1]}]")
            neg_txt = neg_txt.to(device=txt.device).expand(B, -1, -1)
            neg_y = neg_y.to(device=y.device).expand(B, -1)
        cap = self.MAX_ENGINE_BATCH // 2 if guided else self.MAX_ENGINE_BATCH
        stream = self._with_channels(img, img_cond, img_cond_seq) if img.shape[0] <= cap else None
        if img.shape[0] > cap and preview is not None:
            raise ValueError(f"fluxmi: preview / progress / cancellation need a batch that runs in one engine pass (at most {cap} images here)")
        if img.shape[0] > cap:
            # the engine takes at most 32 samples per pass (workspace / modulation-table size); the reference has no num_images limit, so
            # larger batches run as consecutive passes (samples never interact).  EQUAL passes: the engine re-allocates its workspace and
            # re-captures its graph whenever the batch size changes, so 40 = 20 + 20, not 32 + 8.  Only frozen models: a calibrating pass
            # per chunk would advance the F8Linear trial counters once per chunk instead of once per step.
            if self.calibration_state()[0] is False or (cn is not None and cn[0].calibration_state()[0] is False):
                raise ValueError(f"fluxmi: batches larger than {cap} need frozen F8Linear input scales (run the calibration warm-up first)")
            B = img.shape[0]
            n_pass = -(-B // cap)
            per = -(-B // n_pass)
            outs = []
            for i in range(0, B, per):
                sl = slice(i, min(i + per, B))
                pad = per - (sl.stop - sl.start)  # a short last pass is padded with copies of its last sample (same B -> same graph)
                pick = lambda t: torch.cat([t[sl], t[sl.stop - 1:sl.stop].expand(pad, *t.shape[1:])], 0) if pad else t[sl]
                cond = dict(img_cond_seq=pick(img_cond_seq), img_cond_seq_ids=pick(img_cond_seq_ids)) if kontext else {}
                if img_cond is not None:
                    cond["img_cond"] = pick(img_cond)
                if guided:
                    cond.update(neg_txt=pick(neg_txt), neg_y=pick(neg_y), cfg_scale=cfg_scale)
                if attn_groups is not None:
                    halves = attn_groups.chunk(2, 0) if guided else (attn_groups,)
                    cond["attn_groups"] = torch.cat([h if h.shape[0] == 1 else pick(h) for h in halves], 0)
                if inpaint is not None:
                    cond.update(inpaint_x0=pick(inpaint[0]), inpaint_noise=pick(inpaint[1]), inpaint_mask=pick(inpaint[2]),
                                inpaint_thresholds=inpaint[3])
                if cn is not None:
                    cond["controlnet"] = type(controlnet)(cn[0], pick(cn[1]), cn[3], cn[2])
                if ip is not None:  # per sample along dim 1 (scales: dim 0); a guided call's halves are picked separately
                    pick_b = lambda t, dim: torch.cat([pick(h.transpose(0, dim)).transpose(0, dim) for h in t.chunk(2 if guided else 1, dim)], dim)
                    cond["ip_adapter"] = type(ip_adapter)(pick_b(ip[0], 1), pick_b(ip[1], 1), pick_b(ip[2], 0))
                if solver is not None:
                    cond["solver"] = solver
                if solver_noise is not None:  # picked like every per-sample tensor: a padded tail copies the last image's ids
                    cond["solver_noise"] = (solver_noise[0][sl] + solver_noise[0][sl.stop - 1:sl.stop] * pad, solver_noise[1])
                if guidance_shaping is not None:
                    cond["guidance_shaping"] = guidance_shaping
                o = self.denoise(pick(img), pick(img_ids), pick(txt), pick(txt_ids), pick(y), timesteps, guidance=guidance, use_graph=use_graph,
                                 cache_threshold=cache_threshold, cache_max_hits=cache_max_hits, **cond)
                outs.append(o[:per - pad])
            return torch.cat(outs, 0)
        if solver is not None:  # one engine step per evaluation: the program's times, the thresholds of each evaluation's user step
            timesteps = list(solver.times)
            if inpaint is not None and inpaint[3] is not None:
                inpaint = inpaint[:3] + ([inpaint[3][k] for k in solver.step_of_eval],)
        Li = img.shape[1]
        img, img_ids, Lc = self._with_reference(stream, img_ids, img_cond_seq, img_cond_seq_ids)
        img = bf(img).clone()
        if guided:  # the negative branches ride behind the prompt branches: same position ids, the negative prompt's text
            txt, y = torch.cat((txt, neg_txt.to(txt.dtype)), 0), torch.cat((y, neg_y.to(y.dtype)), 0)
            img_ids, txt_ids = torch.cat((img_ids, img_ids), 0), torch.cat((txt_ids, txt_ids), 0)
        txt, y = bf(txt), bf(y)
        self._ensure_engine(img.device)
        with self._lock:
            self._prepare(img, img_ids, txt_ids, txt, Lc)
            if attn_groups is not None and guided and attn_groups.shape[0] == 2 and txt.shape[0] > 2:
                attn_groups = attn_groups.repeat_interleave(txt.shape[0] // 2, 0)  # [pos, neg] -> B x pos, B x neg
            self._set_attn_groups(attn_groups, txt.shape[0], txt.shape[1] + img.shape[1], img.device)
            trial = self._trial_counter()
            t_io = C.c_int(trial if trial is not None else 0)
            ts = (C.c_double * len(timesteps))(*[float(t) for t in timesteps])
            _lib.call("fluxmi_engine_set_step_cache", self._engine, cache_threshold, cache_max_hits)
            self._set_inpaint(inpaint, img.device)
            self._set_solver(solver)
            self._set_solver_noise(solver_noise)
            self._set_guidance(shaping)
            net = self._attach_controlnet(cn, img.device)
            ip_set = False
            pv, rc, ran = None, 0, 0
            try:
                ip_set = self._set_ip_adapter(ip, img.device)
                pv = self._set_preview(preview)
                if guided:
                    rc = _lib.lib.fluxmi_engine_denoise_cfg(self._engine, ops._p(img), ops._p(txt), ops._p(y), float(guidance), float(cfg_scale), ts,
                                                            len(timesteps) - 1, C.byref(t_io), int(use_graph), ops._stream())
                else:
                    rc = _lib.lib.fluxmi_engine_denoise(self._engine, ops._p(img), ops._p(txt), ops._p(y), float(guidance), ts,
                                                        len(timesteps) - 1, C.byref(t_io), int(use_graph), ops._stream())
                if rc != _lib.CANCELLED or pv is None:
                    _lib.check(rc)
                else:
                    cap_ran = (C.c_longlong(0), C.c_int(0))
                    _lib.call("fluxmi_engine_preview_stats", self._engine, C.byref(cap_ran[0]), C.byref(cap_ran[1]))
                    ran = cap_ran[1].value
            finally:
                if pv is not None:
                    _lib.call("fluxmi_engine_set_preview", self._engine, None, 0, 0, 0, 0, 0, None, None)
                self._clear_ip_adapter(ip_set)
                self._release_controlnet(net)
                if solver is not None:
                    self._set_solver(None)
                if shaping is not None:
                    self._set_guidance(None)
            if trial is not None:
                self._advance_calibration(t_io.value)
        if pv is not None and pv["error"] is not None:
            raise pv["error"]
        if rc == _lib.CANCELLED:
            raise GenerationCancelled(preview.eval_offset + ran, preview.n_evaluations)
        if self.in_channels != self.out_channels:
            return img[..., :self.out_channels].contiguous()
        return img[:, :Li].contiguous() if Lc else img

    MAX_EDIT_IMAGES = 16  # fluxmi.flowedit.MAX_IMAGES: the source and the target branch of every image share one engine pass

    def denoise_edit(self, z: Tensor, img_ids: Tensor, src_txt: Tensor, src_y: Tensor, tar_txt: Tensor, tar_y: Tensor, txt_ids: Tensor,
                     timesteps: List[float], n_avg: int = 1, ids=None, eval_offset: int = 0, source_guidance: float = 1.5,
                     guidance: float = 5.5, use_graph: bool = True, preview: PreviewCall | None = None, x0: Tensor | None = None) -> Tensor:
        """FlowEdit's coupled steps (fluxmi.flowedit; Kulikov et al. 2024, Algorithm 1) run natively: the loop of `denoise` -- calibrating
        steps unfused, every later evaluation one replay of a captured hipGraph -- on 2B samples, sample b the SOURCE branch of image b
        (`src_txt` / `src_y`, distilled guidance `source_guidance`) and sample B + b its TARGET branch (`tar_txt` / `tar_y`, `guidance`).
        `z` [B, Li, C]: the edit state; `x0` the init image's latent tokens (None: `z` is x0, the start of an edit).  Every step of
        `timesteps` is coupled: `n_avg` evaluations at its time, each on a fresh coupling zs = (1 - t) x0 + t n, zt = z + zs - x0 written to
        the two halves of the stream, then z moves by dt times the average of (v_target - v_source) (csrc/flowedit.hip: update and next
        coupling in one launch).  `ids` [B, 4] uint32 words per IMAGE (fluxmi.flowedit.edit_ids); the call's first coupling draws at
        `eval_offset`, evaluation j's at eval_offset + j + 1, so a request cut into several calls draws what the uncut one draws.  Returns
        the new z; neither `z` nor `x0` is modified.  `preview`: progress and cancellation only (every = 0), `evaluation` counting model
        evaluations.  At most 16 images; refused under an amax exchange (a process group)."""
        from fluxmi import flowedit

        if getattr(self, "_amax_xchg", None) is not None:
            raise ValueError("fluxmi: FlowEdit is refused under an amax exchange (a process group)")
        preview = self._check_preview(preview)
        if preview is not None and preview.every > 0:
            raise ValueError("fluxmi: FlowEdit has no previews of the edit state (preview.every must be 0: progress and cancellation only)")
        B = z.shape[0]
        if z.ndim != 3 or not 1 <= B <= self.MAX_EDIT_IMAGES:
            raise ValueError(f"fluxmi: FlowEdit takes z [1..{self.MAX_EDIT_IMAGES}, Li, C] (both branches of every image share one engine pass), got "
                             f"{tuple(z.shape)}")
        if self.in_channels != self.out_channels or z.shape[2] != self.in_channels:
            raise ValueError(f"fluxmi: FlowEdit needs a text-to-image model ({self.in_channels} input and {self.out_channels} predicted channels; z has "
                             f"{z.shape[2]})")
        if x0 is None:
            x0 = z
        if tuple(x0.shape) != tuple(z.shape):
            raise ValueError(f"fluxmi: x0 {tuple(x0.shape)} does not match z {tuple(z.shape)}")
        for name, t, want in (("src_txt", src_txt, None), ("tar_txt", tar_txt, tuple(src_txt.shape[1:])), ("src_y", src_y, None),
                              ("tar_y", tar_y, tuple(src_y.shape[1:]))):
            if t.shape[0] not in (1, B) or (want is not None and tuple(t.shape[1:]) != want):
                raise ValueError(f"fluxmi: {name} {tuple(t.shape)}: expected [1 or {B}, ...] with the other branch's sequence length (both "
                                 f"branches run in one batch)")
        program = flowedit.build_program(timesteps, n_avg)
        n = len(program.coef)
        if isinstance(eval_offset, bool) or int(eval_offset) != eval_offset or eval_offset < 0:
            raise ValueError(f"fluxmi: eval_offset={eval_offset!r}: expected an integer >= 0")
        ids = [[int(w) & 0xffffffff for w in row] for row in (ids.tolist() if isinstance(ids, torch.Tensor) else ids or ())]
        if len(ids) != B or any(len(row) != 4 for row in ids):
            raise ValueError(f"fluxmi: ids: expected {B} rows of 4 uint32 words, one row per image (fluxmi.flowedit.edit_ids)")
        bf = lambda t: t.to(device=z.device, dtype=torch.bfloat16).contiguous()
        ex = lambda t: t.to(z.device).expand(B, *t.shape[1:])
        txt, y = bf(torch.cat((ex(src_txt), ex(tar_txt)), 0)), bf(torch.cat((ex(src_y), ex(tar_y)), 0))
        ids2, tids2 = torch.cat((img_ids, img_ids), 0), torch.cat((ex(txt_ids), ex(txt_ids)), 0)
        z, x0 = bf(z).clone(), bf(x0)
        self._ensure_engine(z.device)
        with self._lock:
            self._prepare(z, ids2, tids2, txt, 0)
            self._set_attn_groups(None, txt.shape[0], txt.shape[1] + z.shape[1], z.device)
            _lib.call("fluxmi_engine_set_step_cache", self._engine, 0.0, 0)
            self._set_inpaint(None, z.device)
            self._set_solver(None)
            self._set_guidance(None)
            trial = self._trial_counter()
            t_io = C.c_int(trial if trial is not None else 0)
            coef = (C.c_double * max(1, 4 * n))(*[float(v) for row in program.coef for v in row])
            ctl = (C.c_int * max(1, 2 * n))(*[int(v) for row in program.ctl for v in row])
            flat = (C.c_uint32 * (4 * B))(*[w for row in ids for w in row])
            ts = (C.c_double * max(1, n))(*program.times)
            _lib.call("fluxmi_engine_set_flow_edit", self._engine, ops._p(x0), B, coef, ctl, n, flat, int(eval_offset), float(source_guidance),
                      float(guidance), ops._stream())
            pv, rc, ran = None, 0, 0
            try:
                pv = self._set_preview(preview)
                rc = _lib.lib.fluxmi_engine_denoise_edit(self._engine, ops._p(z), ops._p(txt), ops._p(y), ts, n, C.byref(t_io), int(use_graph),
                                                         ops._stream())
                if rc != _lib.CANCELLED or pv is None:
                    _lib.check(rc)
                else:
                    cap_ran = (C.c_longlong(0), C.c_int(0))
                    _lib.call("fluxmi_engine_preview_stats", self._engine, C.byref(cap_ran[0]), C.byref(cap_ran[1]))
                    ran = cap_ran[1].value
            finally:
                if pv is not None:
                    _lib.call("fluxmi_engine_set_preview", self._engine, None, 0, 0, 0, 0, 0, None, None)
                _lib.call("fluxmi_engine_set_flow_edit", self._engine, None, 0, None, None, 0, None, 0, 0.0, 0.0, None)
            if trial is not None:
                self._advance_calibration(t_io.value)
        if pv is not None and pv["error"] is not None:
            raise pv["error"]
        if rc == _lib.CANCELLED:
            raise GenerationCancelled(preview.eval_offset + ran, preview.n_evaluations)
        return z

    def denoise_windows(self, canvas: Tensor, plan, img_ids: Tensor, txt: Tensor, txt_ids: Tensor, y: Tensor, timesteps: List[float],
                        guidance: float = 3.5, use_graph: bool = True, neg_txt: Tensor | None = None, neg_y: Tensor | None = None,
                        cfg_scale: float = 1.0, preview: PreviewCall | None = None) -> Tensor:
        """Tiled generation (fluxmi.windows; MultiDiffusion, Bar-Tal et al. 2023) run natively: the loop of `denoise` -- calibrating steps
        unfused, every later step one replay of a captured hipGraph -- on the S = N * ny * nx windows of `canvas` [N, Hc, Wc, C] (the token
        grid of the packed latent) that `plan` (a fluxmi.windows.WindowPlan) lays out, sample (n * ny + a) * nx + b window (a, b) of image
        n.  Every window is a stand-alone image to the model: `img_ids` [1, h * w, 3] are the WINDOW's position ids, `txt` / `y` [1 or N,
        ...] are broadcast to an image's windows.  After every evaluation one kernel (csrc/window_step.hip) blends the windows'
        predictions with the plan's weights, steps the canvas once and rebuilds every window from it.  `neg_txt` / `neg_y` (both or
        neither): true classifier-free guidance, 2S samples, `cfg_scale` taken as given and unshaped.  S (guided: 2S) must fit one engine
        pass.  Returns the new canvas; `canvas` is not modified.  `preview`: progress and cancellation only (every = 0).  Refused under an
        amax exchange (a process group)."""
        if getattr(self, "_amax_xchg", None) is not None:
            raise ValueError("fluxmi: tiled generation is refused under an amax exchange (a process group)")
        preview = self._check_preview(preview)
        if preview is not None and preview.every > 0:
            raise ValueError("fluxmi: tiled generation has no previews of the canvas (preview.every must be 0: progress and cancellation only)")
        guided = neg_txt is not None or neg_y is not None
        if guided and (neg_txt is None or neg_y is None):
            raise ValueError("neg_txt and neg_y go together (the negative prompt's T5 sequence and pooled CLIP vector)")
        if canvas.ndim != 4 or tuple(canvas.shape[1:3]) != (plan.Hc, plan.Wc):
            raise ValueError(f"fluxmi: canvas {tuple(canvas.shape)}: expected [N, {plan.Hc}, {plan.Wc}, C] (the plan's token grid)")
        if self.in_channels != self.out_channels or canvas.shape[3] != self.in_channels:
            raise ValueError(f"fluxmi: tiled generation needs a text-to-image model ({self.in_channels} input and {self.out_channels} predicted "
                             f"channels; the canvas has {canvas.shape[3]})")
        N, per = canvas.shape[0], plan.ny * plan.nx
        S, Li = N * per, plan.h * plan.w
        cap = self.MAX_ENGINE_BATCH // 2 if guided else self.MAX_ENGINE_BATCH
        if not 1 <= S <= cap:
            raise ValueError(f"fluxmi: {N} images x {plan.ny} x {plan.nx} windows = {S} samples do not fit one engine pass (at most {cap}"
                             f"{' with a negative prompt' if guided else ''})")
        if img_ids.ndim != 3 or img_ids.shape[0] != 1 or img_ids.shape[1] != Li:
            raise ValueError(f"fluxmi: img_ids {tuple(img_ids.shape)}: expected [1, {Li}, axes], the position ids of ONE window")
        for name, t in (("txt", txt), ("y", y)) + ((("neg_txt", neg_txt), ("neg_y", neg_y)) if guided else ()):
            if t.shape[0] not in (1, N):
                raise ValueError(f"fluxmi: {name} {tuple(t.shape)}: expected [1 or {N}, ...] (one row per image, broadcast to its windows)")
        if guided and (tuple(neg_txt.shape[1:]) != tuple(txt.shape[1:]) or tuple(neg_y.shape[1:]) != tuple(y.shape[1:])):
            raise ValueError(f"fluxmi: neg_txt {tuple(neg_txt.shape)} / neg_y {tuple(neg_y.shape)} must have the prompt's sequence length "
                             f"({tuple(txt.shape)} / {tuple(y.shape)}): both branches run in one batch")
        dev = canvas.device
        bf = lambda t: t.to(device=dev, dtype=torch.bfloat16).contiguous()
        ex = lambda t: t.to(dev).expand(N, *t.shape[1:]).repeat_interleave(per, 0)  # one row per image -> one per window
        B = 2 * S if guided else S
        txt_s, y_s = (torch.cat((ex(txt), ex(neg_txt)), 0), torch.cat((ex(y), ex(neg_y)), 0)) if guided else (ex(txt), ex(y))
        txt_s, y_s = bf(txt_s), bf(y_s)
        ids_s, tids_s = img_ids.to(dev).expand(B, -1, -1), txt_ids[:1].to(dev).expand(B, -1, -1)
        canvas = bf(canvas).clone()
        stream_like = canvas.new_empty((B, Li, canvas.shape[3]))  # (shape only: the engine owns the stream)
        row0 = (C.c_int * plan.ny)(*plan.row0)
        col0 = (C.c_int * plan.nx)(*plan.col0)
        wy = (C.c_float * (plan.ny * plan.Hc))(*plan.Ny.reshape(-1).tolist())
        wx = (C.c_float * (plan.nx * plan.Wc))(*plan.Nx.reshape(-1).tolist())
        self._ensure_engine(dev)
        with self._lock:
            self._prepare(stream_like, ids_s, tids_s, txt_s, 0)
            self._set_attn_groups(None, B, txt_s.shape[1] + Li, dev)
            _lib.call("fluxmi_engine_set_step_cache", self._engine, 0.0, 0)
            self._set_inpaint(None, dev)
            self._set_solver(None)
            self._set_guidance(None)
            trial = self._trial_counter()
            t_io = C.c_int(trial if trial is not None else 0)
            ts = (C.c_double * len(timesteps))(*[float(t) for t in timesteps])
            _lib.call("fluxmi_engine_set_windows", self._engine, N, plan.Hc, plan.Wc, plan.h, plan.w, plan.ny, plan.nx, row0, col0, wy, wx,
                      ops._stream())
            pv, rc, ran = None, 0, 0
            try:
                pv = self._set_preview(preview)
                rc = _lib.lib.fluxmi_engine_denoise_windows(self._engine, ops._p(canvas), ops._p(txt_s), ops._p(y_s), float(guidance), int(guided),
                                                            float(cfg_scale), ts, len(timesteps) - 1, C.byref(t_io), int(use_graph), ops._stream())
                if rc != _lib.CANCELLED or pv is None:
                    _lib.check(rc)
                else:
                    cap_ran = (C.c_longlong(0), C.c_int(0))
                    _lib.call("fluxmi_engine_preview_stats", self._engine, C.byref(cap_ran[0]), C.byref(cap_ran[1]))
                    ran = cap_ran[1].value
            finally:
                if pv is not None:
                    _lib.call("fluxmi_engine_set_preview", self._engine, None, 0, 0, 0, 0, 0, None, None)
                _lib.call("fluxmi_engine_set_windows", self._engine, 0, 0, 0, 0, 0, 0, 0, None, None, None, None, None)
            if trial is not None:
                self._advance_calibration(t_io.value)
        if pv is not None and pv["error"] is not None:
            raise pv["error"]
        if rc == _lib.CANCELLED:
            raise GenerationCancelled(preview.eval_offset + ran, preview.n_evaluations)
        return canvas

    def step_cache_log(self):
        """What first-block step caching did in the last `denoise` call (the last pass of a chunked batch): `(ratios, hits)` with
        `ratios` a float32 tensor [frozen steps, samples of the pass] (inf where no reference existed yet: the first frozen step) and `hits` a
        list of bools, one per frozen step.  Empty after a call with `cache_threshold=0`."""
        if self._engine is None:
            return torch.zeros(0, 0), []
        with self._lock:
            n, B = C.c_int(0), C.c_int(0)
            _lib.call("fluxmi_engine_step_cache_log", self._engine, C.byref(n), C.byref(B), None, None, 0)
            if n.value == 0:
                return torch.zeros(0, 0), []
            r = (C.c_float * (n.value * B.value))()
            h = (C.c_ubyte * n.value)()
            _lib.call("fluxmi_engine_step_cache_log", self._engine, C.byref(n), C.byref(B), r, h, n.value)
        return torch.tensor(list(r), dtype=torch.float32).reshape(n.value, B.value), [bool(v) for v in h]

    @classmethod
    def from_pretrained(cls, path: str, dtype: torch.dtype = torch.float16) -> "Flux":
        from safetensors.torch import load_file

        from util import load_config_from_path

        config = load_config_from_path(path)
        with torch.device("meta"):
            klass = cls(config=config, dtype=dtype)
            if not config.prequantized_flow:
                klass.type(dtype)
        ckpt = load_file(config.ckpt_path, device="cpu")
        klass.load_state_dict(ckpt, assign=True)
        return klass.to("cpu")
