"""LoRA fuse / unfuse into the (fp8) flow weights -- the device-side restatement of the reference's
lora_loading.py:476-753 (aredden/flux-fp8-api), config (5) of the benchmark plan.

In scope: dequantise fp8 -> fp32, dW = scale * (alpha/rank) * B @ A in fp32
(including the reference's "uneven rank" chunk-sum for fused qkv), add, round to the flow dtype,
re-quantise with a fresh amax/scale (F8Linear.set_weight_tensor semantics) -- all on the GPU via
libfluxmi (fluxmi_lora_fuse_f8).  Input scales are NOT recalibrated, exactly like the reference.

Beside plain LoRA a module may carry a LyCORIS LoHa (`hada_w1_a / hada_w1_b / hada_w2_a / hada_w2_b`), LoKr (`lokr_w1` or `lokr_w1_a` +
`lokr_w1_b`, `lokr_w2` or `lokr_w2_a` + `lokr_w2_b`) or full delta (`diff`), each with `alpha`; these, and every load of several adapters at
once, go through fluxmi_adapter_fuse_f8: all terms of a module in one pass over its fp8 bytes and ONE re-quantisation.  The reference has
no counterpart.  Tucker factors and `diff_b` are refused by name.

DoRA: a module that also carries `dora_scale` (shape [N, 1] or [N]: one magnitude per output row, axis 0; [1, K]: per input column, axis 1;
anything else is refused by name) is not an additive delta.  The fuse path rescales every row or column of W + dW to its magnitude through
fluxmi_adapter_fuse_dora_f8, in a call of its own, and keeps the factor pair of that call on the LoraWeights record (`.dora`): unloading
inverts with the stored factors, "the same terms, scale negated" would be wrong.  DoRA does not commute with later fuses, so such an adapter
unloads only as the most recently loaded one (check_unload_order).  get_adapter_for_key still returns the delta alone and warns about the
magnitude it leaves out.  No real DoRA checkpoint has been available: the key layout is the public kohya / LyCORIS convention.

Accepted inputs: a dict with BFL-dotted keys `<module>.lora_A.weight / .lora_B.weight / .alpha`
(lora_loading.py:608-612 skips conversion for dicts), a LoraWeights, or a safetensors path holding such
keys, kohya `lora_unet_*` keys, or diffusers `transformer.*` keys (both converted below; the diffusers
conversion is pinned to the reference's convert_diffusers_to_flux_transformer_checkpoint by
tests/golden/g12_lora_diffusers.safetensors, quirks included).
"""
from __future__ import annotations

import re
import warnings
from typing import Optional, OrderedDict, Tuple, TypeAlias, Union

import torch
from torch import nn

from float8_quantize import F8Linear
from fluxmi import ops

path_regex = re.compile(r"/|\\")
# LyCORIS leaves beside `lora_A / lora_B / alpha` (public LyCORIS / ComfyUI key conventions; no real checkpoint has been available to pin them)
_REFUSED_LEAVES = ("hada_t1", "hada_t2", "lokr_t2", "diff_b")
_ADAPTER_LEAVES = ("hada_w1_a", "hada_w1_b", "hada_w2_a", "hada_w2_b", "lokr_w1", "lokr_w1_a", "lokr_w1_b", "lokr_w2", "lokr_w2_a", "lokr_w2_b",
                   "diff") + _REFUSED_LEAVES
_LEAF_RE = re.compile(r"\.(?:" + "|".join(_ADAPTER_LEAVES + ("dora_scale",)) + r")$")
StateDict: TypeAlias = OrderedDict[str, torch.Tensor]


class LoraWeights:  # reference lora_loading.py:21-32
    def __init__(self, weights: StateDict, path: str, name: str = None, scale: float = 1.0) -> None:
        self.path = path
        self.weights = weights
        self.name = name if name else path_regex.split(path)[-1]
        self.scale = scale
        self.dora = {}  # module key -> (factors [2, N or K], axis) of the DoRA fuse that is in the weights now (fuse_adapters)


def get_module_for_key(key: str, model) -> nn.Module:
    module = model
    for part in key.split("."):
        module = getattr(module, part)
    return module


def get_lora_for_key(key: str, lora_weights: dict) -> Optional[Tuple[torch.Tensor, torch.Tensor, Optional[float]]]:
    prefix = key.split(".lora")[0]
    lora_A = lora_weights.get(f"{prefix}.lora_A.weight")
    lora_B = lora_weights.get(f"{prefix}.lora_B.weight")
    alpha = lora_weights.get(f"{prefix}.alpha")
    if lora_A is None or lora_B is None:
        return None
    return lora_A, lora_B, alpha


def _kohya_to_bfl(sd: dict) -> dict:
    """`lora_unet_double_blocks_0_img_attn_qkv.lora_down.weight` -> `double_blocks.0.img_attn.qkv.lora_A.weight`."""
    out = {}
    for k, v in sd.items():
        if not k.startswith("lora_unet_"):
            out[k] = v
            continue
        stem, _, leaf = k[len("lora_unet_"):].partition(".")
        stem = re.sub(r"^(double_blocks|single_blocks)_(\d+)_", r"\1.\2.", stem)
        for a, b in (("img_attn_", "img_attn."), ("txt_attn_", "txt_attn."), ("img_mlp_", "img_mlp."), ("txt_mlp_", "txt_mlp."),
                     ("img_mod_", "img_mod."), ("txt_mod_", "txt_mod."), ("modulation_", "modulation.")):
            stem = stem.replace(a, b)
        leaf = leaf.replace("lora_down", "lora_A").replace("lora_up", "lora_B")
        out[f"{stem}.{leaf}"] = v
    return out


# ---- diffusers ("transformer.*") LoRA files -> BFL module names ------------------------------------------------------------------------
# Behaviour of the reference's convert_diffusers_to_flux_transformer_checkpoint (lora_loading.py:62-432), restated as tables:
#  * a renamed layer takes EVERY key that contains the diffusers stem as a substring (so `.alpha` and bias keys travel with it);
#  * to_q / to_k / to_v (and add_*_proj) of a double block are concatenated along dim 0 into the fused qkv layer's "uneven rank" form
#    A [3r, K], B [3N', r] (which apply_lora then chunk-sums, lora_loading.py:533-541); a missing member is zero-filled with the shape of
#    the first member found; their `.alpha` keys are NOT consumed (the reference leaves them among the "unexpected keys");
#  * a single block needs all of to_q / to_k / to_v / proj_mlp (the reference pops them unconditionally: KeyError otherwise) and becomes
#    linear1 with A [4r, K], B [3H + mlp, r];
#  * norm_out.linear -> final_layer.adaLN_modulation.1 WITHOUT swapping (scale, shift) (the reference defines swap_scale_shift and
#    never calls it).
_DIFFUSERS_TOP = [
    ("time_text_embed.timestep_embedder.linear_1", "time_in.in_layer", False), ("time_text_embed.text_embedder.linear_1", "vector_in.in_layer", False),
    ("time_text_embed.text_embedder.linear_2", "vector_in.out_layer", False),
    ("time_text_embed.guidance_embedder.linear_1", "guidance_in.in_layer", True), ("time_text_embed.guidance_embedder.linear_2", "guidance_in.out_layer", True),
    ("context_embedder", "txt_in", False), ("x_embedder", "img_in", False),
]
_DIFFUSERS_DOUBLE_PRE = [("norm1.linear", "img_mod.lin"), ("norm1_context.linear", "txt_mod.lin")]
_DIFFUSERS_DOUBLE_POST = [
    ("attn.norm_q", "img_attn.norm.query_norm.scale"), ("attn.norm_k", "img_attn.norm.key_norm.scale"),
    ("attn.norm_added_q", "txt_attn.norm.query_norm.scale"), ("attn.norm_added_k", "txt_attn.norm.key_norm.scale"),
    ("ff.net.0.proj", "img_mlp.0"), ("ff.net.2", "img_mlp.2"), ("ff_context.net.0.proj", "txt_mlp.0"), ("ff_context.net.2", "txt_mlp.2"),
    ("attn.to_out.0", "img_attn.proj"), ("attn.to_add_out", "txt_attn.proj"),
]


def _move_layer(out: dict, sd: dict, stem: str, new_stem: str) -> None:
    hit = [k for k in sd if stem in k]
    for k in hit:
        out[k.replace(stem, new_stem)] = sd.pop(k)


def convert_diffusers_to_flux_transformer_checkpoint(diffusers_state_dict, num_layers, num_single_layers, has_guidance=True, prefix=""):
    """diffusers-format Flux LoRA keys -> `<BFL module>.lora_A.weight / .lora_B.weight` (same name, arguments and result as the
    reference's function; consumes `diffusers_state_dict` like it does)."""
    sd, out = diffusers_state_dict, {}
    for stem, new, guidance_only in _DIFFUSERS_TOP:
        if not guidance_only or has_guidance:
            _move_layer(out, sd, prefix + stem, new)
    dtype = device = None  # (carried from the double blocks into the single blocks' zero fills, as in the reference)
    for i in range(num_layers):
        bp = f"{prefix}transformer_blocks.{i}."
        for stem, new in _DIFFUSERS_DOUBLE_PRE:
            _move_layer(out, sd, bp + stem, f"double_blocks.{i}.{new}")
        found, shape = {}, {"img": None, "txt": None}
        for comp in ("to_q", "to_k", "to_v", "add_q_proj", "add_k_proj", "add_v_proj"):
            ka, kb = f"{bp}attn.{comp}.lora_A.weight", f"{bp}attn.{comp}.lora_B.weight"
            if ka in sd and kb in sd:
                a, b = sd.pop(ka), sd.pop(kb)
                found[comp] = (a, b)
                stream = "txt" if comp.startswith("add_") else "img"
                if shape[stream] is None:
                    shape[stream] = (a.shape, b.shape)
                    dtype, device = a.dtype, a.device
        for stream, comps in (("img", ("to_q", "to_k", "to_v")), ("txt", ("add_q_proj", "add_k_proj", "add_v_proj"))):
            if shape[stream] is None:
                continue
            parts = [found.get(c) or (torch.zeros(shape[stream][0], dtype=dtype, device=device), torch.zeros(shape[stream][1], dtype=dtype, device=device))
                     for c in comps]
            out[f"double_blocks.{i}.{stream}_attn.qkv.lora_A.weight"] = torch.cat([pa for pa, _ in parts], dim=0)
            out[f"double_blocks.{i}.{stream}_attn.qkv.lora_B.weight"] = torch.cat([pb for _, pb in parts], dim=0)
        for stem, new in _DIFFUSERS_DOUBLE_POST:
            _move_layer(out, sd, bp + stem, f"double_blocks.{i}.{new}")
    for i in range(num_single_layers):
        bp = f"{prefix}single_transformer_blocks.{i}."
        _move_layer(out, sd, bp + "norm.linear", f"single_blocks.{i}.modulation.lin")
        parts = [(sd.pop(f"{bp}{c}.lora_A.weight"), sd.pop(f"{bp}{c}.lora_B.weight")) for c in ("attn.to_q", "attn.to_k", "attn.to_v", "proj_mlp")]
        out[f"single_blocks.{i}.linear1.lora_A.weight"] = torch.cat([pa for pa, _ in parts], dim=0)
        out[f"single_blocks.{i}.linear1.lora_B.weight"] = torch.cat([pb for _, pb in parts], dim=0)
        _move_layer(out, sd, bp + "proj_out", f"single_blocks.{i}.linear2")
    _move_layer(out, sd, prefix + "proj_out", "final_layer.linear")  # (weight and bias stems coincide)
    _move_layer(out, sd, prefix + "norm_out.linear", "final_layer.adaLN_modulation.1")
    return out


def resolve_lora_state_dict(lora_weights: dict, has_guidance: bool = True):
    """reference lora_loading.py:580-606: file contents -> (module stems, BFL-keyed weights); 19 / 38 blocks are hard-coded there too."""
    if any(k.startswith("transformer.") for k in lora_weights):
        lora_weights = convert_diffusers_to_flux_transformer_checkpoint(dict(lora_weights), 19, 38, has_guidance=has_guidance, prefix="transformer.")
    else:
        lora_weights = _kohya_to_bfl({k: v for k, v in lora_weights.items() if "lora" in k or _LEAF_RE.search(k)})
    return _keys_without_ab(lora_weights), lora_weights


def _keys_without_ab(lora_weights: dict):
    return sorted({_LEAF_RE.sub("", k).replace(".lora_A.weight", "").replace(".lora_B.weight", "").replace(".lora_A", "").replace(".lora_B", "")
                   .replace(".alpha", "") for k in lora_weights.keys()})


def _resolve(lora_path, has_guidance: bool = True):
    if isinstance(lora_path, LoraWeights):
        return lora_path.weights, lora_path.scale
    if isinstance(lora_path, dict):
        return lora_path, None
    from safetensors.torch import load_file

    return resolve_lora_state_dict(load_file(lora_path, "cpu"), has_guidance)[1], None


def _prescaled_A(lora_A, lora_B, alpha, device):
    """w_up = lora_A (fp32) * alpha / rank  (reference lora_loading.py:519-530); returns (A', n_chunks, rank)."""
    rank = lora_B.shape[1]
    if alpha is None:
        alpha = rank
    a = lora_A.to(dtype=torch.float32, device=device)
    if alpha != rank:
        a = a * alpha / rank
    uneven = lora_B.shape[1] != lora_A.shape[0]
    chunks = int(lora_A.shape[0] / lora_B.shape[1]) if uneven else 1
    return a.contiguous(), chunks, rank


def get_adapter_for_key(key: str, lora_weights: dict, device=None) -> Optional[ops.Delta]:
    """The delta term of module `key` at adapter scale 1, or None when the dict holds no adapter for it.  Plain LoRA keeps the reference's
    arithmetic (alpha / rank folded into lora_A).  LoHa / LoKr / full deltas follow the LyCORIS key layout and ComfyUI's loading rule: the
    factor scale is alpha / rank when a decomposed factor gives a rank, else 1; decomposed LoKr factors are multiplied out here."""
    if f"{key}.dora_scale" in lora_weights:
        warnings.warn(f"adapter key {key}.dora_scale is ignored: DoRA is not supported, the module is fused without its magnitude vector")
    return _delta_for_key(key, lora_weights, device)


def _delta_for_key(key: str, lora_weights: dict, device=None) -> Optional[ops.Delta]:
    for leaf in _REFUSED_LEAVES:
        if f"{key}.{leaf}" in lora_weights:
            raise ValueError(f"adapter key {key}.{leaf}: Tucker-decomposed factors (hada_t1 / hada_t2 / lokr_t2) and bias deltas (diff_b) are not supported")

    def get(leaf):
        t = lora_weights.get(f"{key}.{leaf}")
        return None if t is None else t.to(dtype=torch.float32, device=device)

    alpha = lora_weights.get(f"{key}.alpha")
    alpha = None if alpha is None else float(alpha)
    lora_sd = get_lora_for_key(key, lora_weights)
    if lora_sd is not None:
        a, chunks, _ = _prescaled_A(lora_sd[0], lora_sd[1], lora_sd[2], device)
        return ops.Delta("lora", (lora_sd[1].to(dtype=torch.float32, device=device), a), 1.0, chunks)
    hada = [get(leaf) for leaf in ("hada_w1_a", "hada_w1_b", "hada_w2_a", "hada_w2_b")]
    if all(t is not None for t in hada):
        rank = hada[1].shape[0]
        return ops.Delta("loha", tuple(hada), alpha / rank if alpha is not None else 1.0)
    kron, rank = [], None
    for w in ("lokr_w1", "lokr_w2"):
        full, fa, fb = get(w), get(w + "_a"), get(w + "_b")
        if full is None and fa is not None and fb is not None:
            full, rank = torch.mm(fa, fb), fb.shape[0]
        kron.append(full)
    if all(t is not None for t in kron):
        return ops.Delta("lokr", tuple(kron), alpha / rank if alpha is not None and rank is not None else 1.0)
    diff = get("diff")
    return None if diff is None else ops.Delta("full", (diff,), 1.0)


def get_dora_for_key(key: str, lora_weights: dict, N: int, K: int, device=None):
    """What the fuse path takes for module `key` ([N, K]): (delta at adapter scale 1, magnitude, axis); magnitude and axis are None for a module
    without `dora_scale`.  [N, 1] or [N] is one magnitude per output row (axis 0, also a 1-D vector with N == K), [1, K] one per input column."""
    d = _delta_for_key(key, lora_weights, device)
    m = lora_weights.get(f"{key}.dora_scale")
    if m is None:
        return d, None, None
    if d is None:
        raise ValueError(f"adapter key {key}.dora_scale: a magnitude vector without a delta for its module")
    shape = tuple(m.shape)
    if shape in ((N, 1), (N,)):
        axis = 0
    elif shape == (1, K):
        axis = 1
    else:
        raise ValueError(f"adapter key {key}.dora_scale: shape {list(shape)} is neither [{N}, 1] / [{N}] (one magnitude per output row) nor [1, {K}] "
                         f"(one per input column) of the [{N}, {K}] weight")
    return d, m.to(dtype=torch.float32, device=device).reshape(-1).contiguous(), axis


@torch.inference_mode()
def _fuse_terms(module: nn.Module, terms) -> None:
    """every term of one module in ONE re-quantisation (eight terms per call: FLUXMI_MAX_DELTA_TERMS)"""
    if isinstance(module, F8Linear):
        if len(terms) == 1 and terms[0].kind == "lora":  # a plain LoRA on its own keeps the reference-shaped path and its bits
            d = terms[0]
            ops.lora_fuse_f8(module.float8_data, module.scale, module.scale_reciprocal, d.factors[0].contiguous(), d.factors[1], d.scale, n_chunks=d.n_chunks)
            return
        for i in range(0, len(terms), ops.MAX_DELTA_TERMS):
            ops.adapter_fuse_f8(module.float8_data, module.scale, module.scale_reciprocal, terms[i:i + ops.MAX_DELTA_TERMS])
    else:  # un-quantised nn.Linear: one-off weight surgery in fp32 on the device (plumbing, not hot path)
        w = module.weight.data
        module.weight.data = (w.float() + sum(d.dense() for d in terms)).to(w.dtype)


@torch.inference_mode()
def _fuse_dora(module: nn.Module, term, magnitude, axis: int, strength: float, factors=None):
    """one DoRA call on one module: APPLY (factors None) -> the factor pair [2, N or K]; REMOVE with the pair an APPLY returned"""
    if isinstance(module, F8Linear):
        if factors is None:
            return ops.adapter_fuse_dora_f8(module.float8_data, module.scale, module.scale_reciprocal, [term], magnitude, axis, strength)
        ops.adapter_unfuse_dora_f8(module.float8_data, module.scale, module.scale_reciprocal, [term], factors, axis)
        return factors
    w, D = module.weight.data.float(), term.dense()  # un-quantised nn.Linear: include/fluxmi.h's formula as fp32 surgery (plumbing)
    if factors is None:
        b = strength * (magnitude / ((w + D).norm(dim=1 - axis) + 2.0 ** -23))
        a, b = (1.0 - strength) + b, b
        factors = torch.stack([a, b])
    else:
        a, b = 1.0 / factors[0], -(factors[1] / factors[0])
    a, b = (a[:, None], b[:, None]) if axis == 0 else (a[None, :], b[None, :])
    module.weight.data = (a * w + b * D).to(module.weight.dtype)
    return factors


def _module_device(module: nn.Module):
    return module.float8_data.device if isinstance(module, F8Linear) else module.weight.device


@torch.inference_mode()
def fuse_adapters(model, adapters, dora_remove=None):
    """adapters: [(BFL-keyed weights, scale)].  Gathers, per module, the terms of every adapter and fuses them together: ONE re-quantisation
    for the additive terms.  A module with a magnitude vector (DoRA) is fused in a call of its own, in adapter list order, with the adapter's
    scale as the strength: DoRA does not add, so a list re-quantises such a module once per DoRA adapter, plus once for the additive terms on
    either side of it.  Returns, per adapter, {module key: (factors, axis)} of its DoRA calls.  dora_remove (the same structure, or None per
    adapter): the DoRA modules of that adapter are taken OUT with the stored factors instead (its additive modules take `scale` as given)."""
    per_module, out = {}, [{} for _ in adapters]
    for i, (lora_weights, scale) in enumerate(adapters):
        for key in _keys_without_ab(lora_weights):
            if get_lora_for_key(key, lora_weights) is None and not any(f"{key}.{leaf}" in lora_weights for leaf in _ADAPTER_LEAVES):
                continue  # (before the module lookup: converted files carry keys of no module, as in the reference)
            module = get_module_for_key(key, model)
            N, K = (module.float8_data if isinstance(module, F8Linear) else module.weight).shape
            d, magnitude, axis = get_dora_for_key(key, lora_weights, N, K, _module_device(module))
            if d is None:
                continue
            calls = per_module.setdefault(key, (module, []))[1]
            if magnitude is not None:
                stored = (dora_remove[i] or {}).get(key) if dora_remove else None
                if dora_remove and stored is None:
                    raise ValueError(f"adapter key {key}.dora_scale: a DoRA module is taken out with the factors its fuse returned, and none are recorded")
                calls.append((i, key, d, magnitude, axis, scale, stored))
            elif calls and isinstance(calls[-1], list):
                calls[-1].append(d.scaled(scale))
            else:
                calls.append([d.scaled(scale)])
    for module, calls in per_module.values():
        for call in calls:
            if isinstance(call, list):
                _fuse_terms(module, call)
            else:
                i, key, d, magnitude, axis, scale, stored = call
                out[i][key] = (_fuse_dora(module, d, magnitude, axis, scale, None if stored is None else stored[0]), axis)
    if hasattr(model, "rebind_weights"):
        model.rebind_weights()
    return out


def _guidance(model) -> bool:
    return bool(getattr(getattr(model, "params", None), "guidance_embed", True))


@torch.inference_mode()
def apply_lora_to_model(model, lora_path, lora_scale: float = 1.0, return_lora_resolved: bool = False):
    """reference lora_loading.py:634-693."""
    lora_weights, _ = _resolve(lora_path, _guidance(model))
    dora = fuse_adapters(model, [(lora_weights, lora_scale)])[0]
    if isinstance(lora_path, LoraWeights):
        lora_path.dora = dora  # (a DoRA adapter unloads only through its record: remove_lora_from_module)
    if return_lora_resolved:
        return model, lora_weights
    return model


@torch.inference_mode()
def apply_loras_to_model(model, loras):
    """loras: [(path, dict or LoraWeights, scale)] -> the resolved weights of each, after ONE fuse per module over all their additive terms
    (fuse_adapters: DoRA modules take a call of their own; a LoraWeights member records their factors)"""
    resolved = [(_resolve(path, _guidance(model))[0], scale) for path, scale in loras]
    for (path, _), dora in zip(loras, fuse_adapters(model, resolved)):
        if isinstance(path, LoraWeights):
            path.dora = dora
    return [w for w, _ in resolved]


@torch.inference_mode()
def remove_lora_from_module(model, lora_path, lora_scale: float = 1.0):
    """reference lora_loading.py:696-753: subtract the same delta and re-quantise (lossy through fp8, as there).  The DoRA modules of a
    LoraWeights record are inverted with the factors their fuse left on it; a stored factor a_i that is zero or not finite (a row scaled to
    nothing cannot be scaled back) refuses the whole unload by name, before anything is touched: one device-to-host check."""
    lora_weights, stored_scale = _resolve(lora_path, _guidance(model))
    if stored_scale is not None:
        lora_scale = stored_scale
    dora = dict(getattr(lora_path, "dora", None) or {})
    if dora:
        bad = torch.stack([((f[0] == 0) | ~torch.isfinite(f[0])).any() for f, _ in dora.values()]).cpu()
        if bool(bad.any()):
            keys = [k for k, x in zip(dora, bad.tolist()) if x]
            raise ValueError(f"unload of {getattr(lora_path, 'name', 'the adapter')!r}: the stored DoRA factors of {keys} hold a zero or non-finite "
                             "scale, which has no inverse")
    fuse_adapters(model, [(lora_weights, -lora_scale)], dora_remove=[dora])
    if isinstance(lora_path, LoraWeights):
        lora_path.dora = {}
    return model


def check_unload_order(loras, idx: int) -> None:
    """DoRA does not commute with later fuses: raises a ValueError that names the adapter to unload first when loras[idx] (a list of
    LoraWeights in load order) is a DoRA adapter with anything loaded after it, or shares a module with a DoRA adapter loaded after it."""
    rec, later = loras[idx], loras[idx + 1:]
    if rec.dora and later:
        raise ValueError(f"{rec.name!r} is a DoRA adapter and not the most recently loaded one: unload {later[-1].name!r} first")
    mine = set(_keys_without_ab(rec.weights))
    for other in reversed(later):
        if other.dora and mine & set(_keys_without_ab(other.weights)):
            raise ValueError(f"{rec.name!r} was loaded before the DoRA adapter {other.name!r}, which rescaled modules they share: unload {other.name!r} first")
