"""Operator-level host wrappers: torch CUDA(HIP) tensors in, libfluxmi kernels underneath.

PyTorch is plumbing only (device memory + current stream).  Every function launches on
`torch.cuda.current_stream()` and never synchronises.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import E4M3, E5M2, GemmGroup, call

F8_DTYPES = {torch.float8_e4m3fn: E4M3, torch.float8_e5m2: E5M2}
F8_MAX = {E4M3: 448.0, E5M2: 57344.0}


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _req(t: torch.Tensor, dtype=None, name="tensor"):
    if not t.is_cuda:
        raise RuntimeError(f"fluxmi: {name} must live on the GPU (got {t.device}); there is no CPU path")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"fluxmi: {name} must be {dtype}, got {t.dtype}")
    return t


def fmt_of(dtype) -> int:
    return F8_DTYPES[dtype]


def dtype_of(fmt: int):
    return torch.float8_e5m2 if fmt == E5M2 else torch.float8_e4m3fn


# ---- quantisation ------------------------------------------------------------------------------
def quantize_act(x: torch.Tensor, scale: torch.Tensor, fmt: int = E5M2, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float8_quantize.py:217-218 + cast.  x: bf16 [..., K] (last dim contiguous)."""
    _req(x, torch.bfloat16, "x")
    x2 = x.reshape(-1, x.shape[-1])
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    if out is None:
        out = torch.empty(x2.shape, dtype=dtype_of(fmt), device=x.device)
    call("fluxmi_quantize_act", _p(x2), _p(out), _p(scale), x2.shape[0], x2.shape[1], x2.stride(0), out.stride(0), fmt, _stream())
    return out.view(*x.shape[:-1], x.shape[-1])


def amax(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _req(x, torch.bfloat16, "x")
    x2 = x.reshape(-1, x.shape[-1])
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    if out is None:
        out = torch.zeros((), dtype=torch.float32, device=x.device)
    call("fluxmi_amax", _p(x2), _p(out), x2.shape[0], x2.shape[1], x2.stride(0), _stream())
    return out


def calib_update(amax_t, trials, scale, scale_recip, trial_index: int, num_trials: int, max_val: float) -> None:
    call("fluxmi_calib_update", _p(amax_t), _p(trials), _p(scale), _p(scale_recip), trial_index, num_trials, max_val, _stream())


def quantize_weight(w: torch.Tensor, fmt: int = E4M3):
    """F8Linear.quantize_weight (float8_quantize.py:195-207) -> (float8_data, scale, scale_reciprocal)."""
    _req(w, torch.bfloat16, "weight")
    w = w.contiguous()
    q = torch.empty(w.shape, dtype=dtype_of(fmt), device=w.device)
    tmp = torch.zeros(3, dtype=torch.float32, device=w.device)
    call("fluxmi_quantize_weight", _p(w), _p(q), _p(tmp[0:1]), _p(tmp[1:2]), _p(tmp[2:3]), w.shape[0], w.shape[1], fmt, _stream())
    return q, tmp[1].clone(), tmp[2].clone()


def dequant(q: torch.Tensor, scale_recip: torch.Tensor) -> torch.Tensor:
    out = torch.empty(q.shape, dtype=torch.float32, device=q.device)
    call("fluxmi_dequant", _p(q), _p(out), _p(scale_recip), q.numel(), fmt_of(q.dtype), _stream())
    return out


def lora_fuse_f8(w8: torch.Tensor, w_scale: torch.Tensor, w_scale_recip: torch.Tensor, lora_B: torch.Tensor,
                 lora_A: torch.Tensor, lora_scale: float, n_chunks: int = 1) -> None:
    """In-place LoRA fuse + re-quantise of an e4m3 weight (lora_loading.py:509-577,615-631,686-687)."""
    N, K = w8.shape
    R = lora_B.shape[1]
    work = torch.empty(2 * N * K, dtype=torch.float32, device=w8.device)
    tmp = torch.zeros(1, dtype=torch.float32, device=w8.device)
    if w8.dtype != torch.float8_e4m3fn:
        raise TypeError(f"fluxmi: LoRA fuse needs float8_e4m3fn weights (the GEMM kernels fix the weight operand format), got {w8.dtype}")
    call("fluxmi_lora_fuse_f8", _p(w8), _p(w_scale), _p(w_scale_recip), _p(lora_B.float().contiguous()),
         _p(lora_A.float().contiguous()), N, K, R, n_chunks, float(lora_scale), _p(work), _p(tmp), _stream())


# ---- linear ----------------------------------------------------------------------------------------
def make_group(A, W, bias, sa_recip, sb_recip, Cout, M, lda, ldc, *, C2=None, ldc2=0, gate=None, resid=None, ldr=0,
               q_scale=None, split_n=0, c2_col0=0, vt_out=None, vt_ld=0, tok0=0, vt_rows=0, kv_col0=0, heads=0, k_out=None, pe=None,
               k_norm=None, k_rows=0, q_lut=None, k_f16=False, W_pairs=None, a_pairs=False, c8_pairs=False) -> GemmGroup:
    g = GemmGroup()
    g.q_lut = q_lut
    g.W_pairs = W_pairs
    g.a_pairs, g.c8_pairs = int(a_pairs), int(c8_pairs)
    g.k_f16 = int(k_f16)
    g.vt_out, g.k_out, g.pe, g.k_norm = vt_out, k_out, pe, k_norm
    g.vt_ld, g.k_rows, g.tok0, g.vt_rows, g.kv_col0, g.heads = vt_ld, k_rows, tok0, vt_rows, kv_col0, heads
    g.A, g.W, g.bias, g.sa_recip, g.sb_recip = A, W, bias, sa_recip, sb_recip
    g.C, g.C2, g.gate, g.resid, g.q_scale = Cout, C2, gate, resid, q_scale
    g.lda, g.ldc, g.ldc2, g.ldr, g.M, g.split_n, g.c2_col0 = lda, ldc, ldc2, ldr, M, split_n, c2_col0
    return g


def gemm_grouped(groups: Sequence[GemmGroup], N: int, K: int, is_fp8: bool, act_fmt: int, epilogue: int, tile_cfg: int = -1) -> None:
    arr = (GemmGroup * len(groups))(*groups)
    call("fluxmi_gemm_grouped", arr, len(groups), N, K, int(is_fp8), act_fmt, epilogue, tile_cfg, _stream())


def gemm_plan(groups: Sequence[GemmGroup], N: int, K: int, is_fp8: bool, act_fmt: int, epilogue: int, batch: int = 1):
    """fluxmi_gemm_plan: the launches gemm_grouped(tile_cfg=-1) would issue for these groups under the current tuning, as a list of dicts
    with kind ("tile", "generic", "splitk"), cfg (tile config or -1), S (split-K slices or 0) and groups (indices into `groups`, in
    launch order).  Host arithmetic only -- works without a GPU, the groups' pointers are never followed."""
    arr = (GemmGroup * len(groups))(*groups)
    cap = 5 * len(groups)
    raw, n = (C.c_int * cap)(), C.c_int()
    call("fluxmi_gemm_plan", arr, len(groups), N, K, int(is_fp8), act_fmt, epilogue, batch, raw, cap, C.byref(n))
    v, i, launches = list(raw[: n.value]), 0, []
    while i < len(v):
        kind, cfg, S, ng = v[i:i + 4]
        launches.append(dict(kind=("tile", "generic", "splitk")[kind], cfg=cfg, S=S, groups=v[i + 4:i + 4 + ng]))
        i += 4 + ng
    return launches


def pair_rows(w: torch.Tensor) -> torch.Tensor:
    """[R, C] (1-byte or 2-byte elements, row bytes % 64 == 0, R even) -> the same bytes in the row-pair layout [R/2][row_bytes/64][2][64]
    (fluxmi_gemm_group_t.W_pairs), as a tensor of w's shape and dtype."""
    assert w.dim() == 2 and w.is_contiguous()
    out = torch.empty_like(w)
    call("fluxmi_pair_rows", _p(w), _p(out), w.shape[0], w.shape[1] * w.element_size(), _stream())
    return out


def build_quant_lut(scale: torch.Tensor, fmt: int = E5M2, act: int = 1) -> torch.Tensor:
    """64 KiB table bf16 bit pattern -> fp8 byte of quantise(act(x)) (act: 0 none, 1 gelu-tanh, 2 silu) for a frozen input scale."""
    lut = torch.empty(65536, dtype=torch.uint8, device=scale.device)
    call("fluxmi_build_quant_lut", _p(scale), fmt, act, _p(lut), _stream())
    return lut


def linear(x, W, bias=None, sa_recip=None, sb_recip=None, *, epilogue=_lib.EPI_BF16, gate=None, resid=None, q_scale=None,
           out=None, out2=None, split_n=0, c2_col0=0, tile_cfg=-1, out_fmt=E5M2, q_lut=None):
    """One (F8)Linear: x [M,K] fp8 or bf16, W [N,K].  Returns the primary output tensor."""
    is_fp8 = W.dtype in F8_DTYPES
    M, K = x.shape
    N = W.shape[0]
    act_fmt = fmt_of(x.dtype) if is_fp8 else out_fmt
    fp8_out = epilogue in (_lib.EPI_GELU_QUANT, _lib.EPI_QUANT, _lib.EPI_SILU_QUANT)
    n_primary = split_n if epilogue == _lib.EPI_SPLIT else N
    if out is None:
        out = torch.empty((M, n_primary), dtype=dtype_of(act_fmt) if fp8_out else torch.bfloat16, device=x.device)
    g = make_group(_p(x), _p(W), _p(bias), _p(sa_recip), _p(sb_recip), _p(out), M, x.stride(0), out.stride(0),
                   C2=_p(out2), ldc2=out2.stride(0) if out2 is not None else 0, gate=_p(gate), resid=_p(resid),
                   ldr=resid.stride(0) if resid is not None else 0, q_scale=_p(q_scale), split_n=split_n, c2_col0=c2_col0, q_lut=_p(q_lut))
    gemm_grouped([g], N, K, is_fp8, act_fmt, epilogue, tile_cfg)
    return out


def gemv(x, W, bias=None, in_scale=None, sa_recip=None, sb_recip=None, pre_silu=False, act_fmt=E5M2, out=None):
    B, K = x.shape
    N = W.shape[0]
    if out is None:
        out = torch.empty((B, N), dtype=torch.bfloat16, device=x.device)
    call("fluxmi_gemv", _p(x), x.stride(0), _p(W), _p(bias), _p(in_scale), _p(sa_recip), _p(sb_recip), _p(out), out.stride(0),
         B, N, K, int(W.dtype in F8_DTYPES), act_fmt, int(pre_silu), _stream())
    return out


# ---- block elementwise ---------------------------------------------------------------------------------
def ln_modulate(x, shift0, scale0, shift1=None, scale1=None, split=None, q_scale0=None, q_scale1=None, fmt=E5M2, out=None, out_pairs=False):
    """x [B,L,H] bf16; shift/scale [B,H] (row stride = mod_bstride).  fp8 output iff q_scale0 is given.  x and `out` [B,L,H] may be column
    slices of wider [B,L,W] buffers (batch stride = L * row stride).  out_pairs: the fp8 output in the row-pair layout (pair_rows) over
    the B * L rows; the library refuses it where the streaming kernel cannot write it (fluxmi_ln_modulate_pairs)."""
    B, L, H = x.shape
    split = L if split is None else split
    shift1 = shift0 if shift1 is None else shift1
    scale1 = scale0 if scale1 is None else scale1
    out_fp8 = q_scale0 is not None
    q_scale1 = q_scale0 if q_scale1 is None else q_scale1
    if out is None:
        out = torch.empty((B, L, H), dtype=dtype_of(fmt) if out_fp8 else torch.bfloat16, device=x.device)
    for t, name in ((x, "x"), (out, "out")):
        if tuple(t.shape) != (B, L, H) or t.stride(2) != 1 or (B > 1 and t.stride(0) != L * t.stride(1)):
            raise ValueError(f"ln_modulate: {name} must be [B, L, H] with unit column stride and batch stride L * row stride")
    args = (_p(x), x.stride(1), _p(out), out.stride(1), _p(shift0), _p(scale0), _p(shift1), _p(scale1), shift0.stride(0),
            _p(q_scale0), _p(q_scale1), B, L, split, H, int(out_fp8), fmt)
    if out_pairs:
        call("fluxmi_ln_modulate_pairs", *args, 1, _stream())
    else:
        call("fluxmi_ln_modulate", *args, _stream())
    return out


def act(x, mode: int, out=None):
    """out: a preallocated [rows, cols] bf16 tensor (a column slice of a wider buffer is fine), returned as it is"""
    x2 = x.reshape(-1, x.shape[-1])
    y = torch.empty(x2.shape, dtype=x.dtype, device=x.device) if out is None else out
    call("fluxmi_act", _p(x2), _p(y), x2.shape[0], x2.shape[1], x2.stride(0), y.stride(0), mode, _stream())
    return y.view(x.shape) if out is None else out


def _rows3(t, name):
    """[B, L, H], unit column stride, rows of all batch elements at one stride (dense, or a column slice of a wider [B, L, W] buffer)"""
    B, L, _ = t.shape
    if t.stride(2) != 1 or (B > 1 and t.stride(0) != L * t.stride(1)):
        raise ValueError(f"gate_residual: {name} must be [B, L, H] with unit column stride and batch stride L * row stride")
    return t.stride(1)


def gate_residual(x, y, gate, out=None):
    """out = x + gate[b] * y.  x, y, out [B,L,H] may be column slices of wider buffers; gate [B,H] with any batch stride."""
    B, L, H = x.shape
    if out is None:
        out = torch.empty((B, L, H), dtype=x.dtype, device=x.device)
    call("fluxmi_gate_residual", _p(x), _p(y), _p(gate), _p(out), B, L, H, _rows3(x, "x"), _rows3(y, "y"), _rows3(out, "out"),
         gate.stride(0), _stream())
    return out


def add(a, b, out=None):
    z = torch.empty_like(a) if out is None else out
    call("fluxmi_add", _p(a), _p(b), _p(z), a.numel(), _stream())
    return z


def add_bcast(a, b, out=None):
    """z[r, :] = a[r, :] + b[r % nb, :]: a [rows, cols], b [nb, cols], both dense bf16"""
    assert a.dim() == 2 and b.dim() == 2 and a.is_contiguous() and b.is_contiguous() and a.shape[1] == b.shape[1]
    z = torch.empty_like(a) if out is None else out
    assert z.is_contiguous() and z.shape == a.shape
    call("fluxmi_add_bcast", _p(a), _p(b), _p(z), a.shape[0], b.shape[0], a.shape[1], _stream())
    return z


# ---- attention path -------------------------------------------------------------------------------------
def rope_tables_host(axes_dim, theta):
    """Host-side constants, evaluated with the reference's own torch expressions (flux_model.py:50-51)."""
    omega, axis = [], []
    for i, d in enumerate(axes_dim):
        frac = torch.arange(0, d, 2, dtype=torch.float32) / d
        om = 1.0 / (theta ** frac)
        omega.append(om)
        axis += [i] * om.numel()
    return torch.cat(omega).contiguous(), torch.tensor(axis, dtype=torch.int32)


def timestep_freqs_host(half=128, max_period=10000):
    import math
    return torch.exp(-math.log(max_period) * torch.arange(0, half, dtype=torch.float32) / half)


def rope_table(ids: torch.Tensor, axes_dim, theta) -> torch.Tensor:
    """ids bf16 [B,L,3] -> pe bf16 [B,L,64,2] (cos, sin)."""
    om, ax = rope_tables_host(axes_dim, theta)
    om, ax = om.to(ids.device), ax.to(ids.device)
    B, L, n_axes = ids.shape
    pe = torch.empty((B, L, om.numel(), 2), dtype=torch.bfloat16, device=ids.device)
    call("fluxmi_rope_table", _p(ids.contiguous()), _p(om), _p(ax), _p(pe), B * L, n_axes, om.numel(), _stream())
    return pe


def qkv_rope(qkv, pe, q_scale0, k_scale0, q_scale1=None, k_scale1=None, split=None, heads=None, skip_q=False, k_f16=False, out=None):
    """qkv bf16 [B,L,>=3*H*128] -> Q,K [B,H,L,128], VT [B,H,128,Lp].  skip_q: only K and VT (Q is returned as None).
    k_f16: K is returned as float16 (the operand format of the attention kernel's folded schedule; pass it on to attention*).
    out: preallocated contiguous (Q, K, VT) of those shapes and dtypes (Q ignored under skip_q; VT's last dimension is taken as Lp)."""
    B, L, _ = qkv.shape
    split = L if split is None else split
    q_scale1 = q_scale0 if q_scale1 is None else q_scale1
    k_scale1 = k_scale0 if k_scale1 is None else k_scale1
    Lp = (L + 63) // 64 * 64
    if out is not None:
        Q, K, VT = out
        Q = None if skip_q else Q
        Lp = VT.shape[-1]
        for t, shape, dt in ((Q, (B, heads, L, 128), torch.bfloat16), (K, (B, heads, L, 128), torch.float16 if k_f16 else torch.bfloat16),
                             (VT, (B, heads, 128, Lp), torch.bfloat16)):
            if t is not None and (tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous()):
                raise ValueError(f"qkv_rope: out tensors must be contiguous {shape} {dt}, got {tuple(t.shape)} {t.dtype}")
    else:
        K = torch.empty((B, heads, L, 128), dtype=torch.float16 if k_f16 else torch.bfloat16, device=qkv.device)
        Q = None if skip_q else torch.empty((B, heads, L, 128), dtype=torch.bfloat16, device=qkv.device)
        VT = torch.empty((B, heads, 128, Lp), dtype=torch.bfloat16, device=qkv.device)
    call("fluxmi_qkv_rope", _p(qkv), qkv.stride(1), _p(pe), _p(q_scale0), _p(k_scale0), _p(q_scale1), _p(k_scale1), _p(Q), _p(K),
         _p(VT), B, L, Lp, heads, split, int(k_f16), _stream())
    return Q, K, VT


ATTN_GROUPS = 16  # key groups of a token-group mask (include/fluxmi.h, fluxmi_attention_grouped)
ATTN_MASK_FLOOR = -1024.0  # exp2 domain: where a masked row's running maximum starts (M_FLOOR of csrc/attention2.hip)
ATTN_MASK_L_MAX = 12096  # the keys' group codes are staged in LDS behind the K / V^T rings


def attn_descriptors(group: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
    """Per-token descriptors of a token-group mask: group [.., L] in [0, 16) = the token's key group, perm [.., L] = bit set of the groups
    its query admits -> int32 [.., L] holding the bits of FLUXMI_ATTN_DESC(group, perm).  Query i attends key j iff bit group[j] of perm[i]."""
    g, p = group.to(torch.int64), perm.to(torch.int64)
    if g.numel() and (int(g.min()) < 0 or int(g.max()) >= ATTN_GROUPS or int(p.min()) < 0 or int(p.max()) >= 1 << ATTN_GROUPS):
        raise ValueError(f"attn_descriptors: groups must lie in [0, {ATTN_GROUPS}) and permission sets in [0, 2^{ATTN_GROUPS})")
    d = g | (p << 16)
    return torch.where(d >= 1 << 31, d - (1 << 32), d).to(torch.int32)


def attn_groups_allowed(groups: torch.Tensor) -> torch.Tensor:
    """descriptors [B, L] -> bool [B, L, L]: allowed[b, i, j] = query i attends key j (the attn_mask of F.scaled_dot_product_attention)"""
    d = groups.to(torch.int64) & 0xFFFFFFFF
    g, p = d & 15, d >> 16
    return ((p[:, :, None] >> g[:, None, :]) & 1).bool()


def check_attn_groups(groups: torch.Tensor, B: int, L: int) -> torch.Tensor:
    """Shape, dtype and SELF-ADMISSION of a descriptor table (every query admits its own group: no softmax row is empty)."""
    if groups.dtype not in (torch.int32, torch.uint32) or tuple(groups.shape) != (B, L) or not groups.is_contiguous():
        raise ValueError(f"attention groups: need a contiguous int32 / uint32 [B={B}, L={L}] table, got {groups.dtype} {tuple(groups.shape)}")
    d = groups.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    g, p = d & 15, d >> 16
    if bool((d & 0xFFF0).any()):
        raise ValueError("attention groups: bits 4-15 of a descriptor must be zero")
    if not bool(((p >> g) & 1).all()):
        raise ValueError("attention groups: every query must admit its own key group (an empty softmax row otherwise)")
    return groups


def attention(Q, K, VT, q_scale0=None, q_scale1=None, split=None, fmt=E5M2, out=None, col_off=0, groups=None, out_pairs=False):
    """K may be bfloat16 or float16 (float16 selects the folded kernel, see include/fluxmi.h).
    groups: a token-group mask, int32 [B, L] descriptors on the device (attn_descriptors); out_pairs (with groups, fp8 output): rows in
    the row-pair layout (pair_rows).  With groups, L <= 12096, and a row's admitted scores must not all lie below ATTN_MASK_FLOOR + 126
    in the exp2 domain (q . k / sqrt(128) * log2 e; about |q . k| / sqrt(128) < 620): the masked rows' running maximum starts from that
    floor, below it a row sums to l = 0 and comes out inf / nan.  Nothing checks this per call (Q is device data); QK-normed operands
    are two orders of magnitude inside it."""
    B, H, L, _ = Q.shape
    Lp = VT.shape[-1]
    split = L if split is None else split
    out_fp8 = q_scale0 is not None
    q_scale1 = q_scale0 if q_scale1 is None else q_scale1
    if out is None:
        out = torch.empty((B, L, H * 128), dtype=dtype_of(fmt) if out_fp8 else torch.bfloat16, device=Q.device)
    if groups is not None:
        check_attn_groups(groups, B, L)
        call("fluxmi_attention_grouped", _p(Q), _p(K), _p(VT), _p(out), out.stride(1), col_off, int(out_fp8), _p(q_scale0), _p(q_scale1), split,
             B, L, Lp, H, fmt, int(K.dtype == torch.float16), _p(groups), int(out_pairs), _stream())
        return out
    if out_pairs:
        raise ValueError("attention: out_pairs is an argument of the grouped entry (pass groups)")
    call("fluxmi_attention", _p(Q), _p(K), _p(VT), _p(out), out.stride(1), col_off, int(out_fp8), _p(q_scale0), _p(q_scale1), split,
         B, L, Lp, H, fmt, int(K.dtype == torch.float16), _stream())
    return out


def unpair_rows(w: torch.Tensor) -> torch.Tensor:
    """inverse of pair_rows: the row-pair layout [R/2][row_bytes/64][2][64] back to plain rows [R, C]"""
    assert w.dim() == 2 and w.is_contiguous()
    out = torch.empty_like(w)
    call("fluxmi_unpair_rows", _p(w), _p(out), w.shape[0], w.shape[1] * w.element_size(), _stream())
    return out


def attention_plan(B: int, L: int, H: int):
    """fluxmi_attention_plan: None when an attention launch of this shape runs one workgroup per task, else a dict with the balanced
    grid's geometry: n_per_x / full_per_x (tasks per XCD, of which whole), `thin` (the default takes the plan) and `pieces` in launch order (dicts with tloc, pidx, np,
    base, tb, len).  Host arithmetic only -- works without a GPU."""
    import ctypes as C

    n, f, npc = C.c_int(), C.c_int(), C.c_int()
    raw = (C.c_ulonglong * 64)()
    kind = _lib.lib.fluxmi_attention_plan(B, L, H, C.byref(n), C.byref(f), C.byref(npc), raw)
    if not kind:
        return None
    pieces = [dict(tloc=v & 255, pidx=(v >> 8) & 255, np=(v >> 16) & 255, base=(v >> 24) & 255, tb=(v >> 32) & 0xFFFF, len=(v >> 48) & 0xFFFF)
              for v in list(raw)[: npc.value]]
    return dict(n_per_x=n.value, full_per_x=f.value, pieces=pieces, thin=kind == 1)  # thin: what fluxmi_tuning_t.attn_split = 1 takes


def attention_rawq(qkv, pe, qn_scale0, K, VT, qn_scale1=None, q_scale0=None, q_scale1=None, split=None, fmt=E5M2, out=None, col_off=0,
                   groups=None, out_pairs=False):
    """Attention with Q read raw from the qkv GEMM output [B,L,>=H*128] (QKNorm + RoPE applied on load); K, VT from qkv_rope.
    groups / out_pairs: as in attention."""
    B, H, L, _ = K.shape
    Lp = VT.shape[-1]
    split = L if split is None else split
    qn_scale1 = qn_scale0 if qn_scale1 is None else qn_scale1
    out_fp8 = q_scale0 is not None
    q_scale1 = q_scale0 if q_scale1 is None else q_scale1
    if out is None:
        out = torch.empty((B, L, H * 128), dtype=dtype_of(fmt) if out_fp8 else torch.bfloat16, device=K.device)
    if groups is not None:
        check_attn_groups(groups, B, L)
        call("fluxmi_attention_rawq_grouped", _p(qkv), qkv.stride(1), _p(pe), _p(qn_scale0), _p(qn_scale1), _p(K), _p(VT), _p(out),
             out.stride(1), col_off, int(out_fp8), _p(q_scale0), _p(q_scale1), split, B, L, Lp, H, fmt, int(K.dtype == torch.float16),
             _p(groups), int(out_pairs), _stream())
        return out
    if out_pairs:
        raise ValueError("attention_rawq: out_pairs is an argument of the grouped entry (pass groups)")
    call("fluxmi_attention_rawq", _p(qkv), qkv.stride(1), _p(pe), _p(qn_scale0), _p(qn_scale1), _p(K), _p(VT), _p(out), out.stride(1),
         col_off, int(out_fp8), _p(q_scale0), _p(q_scale1), split, B, L, Lp, H, fmt, int(K.dtype == torch.float16), _stream())
    return out


def timestep_embedding(t: torch.Tensor, freqs: torch.Tensor, time_factor: float = 1000.0) -> torch.Tensor:
    B = t.shape[0]
    half = freqs.numel()
    out = torch.empty((B, 2 * half), dtype=torch.bfloat16, device=t.device)
    call("fluxmi_timestep_embedding", _p(t), _p(freqs), _p(out), B, half, time_factor, _stream())
    return out


def euler_(img: torch.Tensor, pred: torch.Tensor, dt: float) -> torch.Tensor:
    dts = torch.tensor([dt], dtype=torch.float32, device=img.device)
    call("fluxmi_euler", _p(img), _p(pred), _p(dts), None, img.numel(), _stream())
    return img


# ---- VAE decoder pieces (NHWC bf16) -------------------------------------------------------------------------------------
def conv3x3_ok(cin: int, cout: int) -> bool:
    """shapes fluxmi_conv3x3 (the implicit-GEMM 3x3 convolution) takes: 64-channel K-steps, 128-column tiles"""
    return cin % 64 == 0 and cout % 128 == 0


def conv3x3(x: torch.Tensor, w2: torch.Tensor, bias=None, upsample: int = 1, resid=None, gate=None) -> torch.Tensor:
    """x [B, Hin, Win, C] bf16 (NHWC), w2 [Cout, 9*C] bf16 with K ordered (dy, dx, c) -> [B, H, W, Cout]: the 3x3 convolution as an IMPLICIT
    GEMM (no patch matrix).  `upsample` as in im2col3x3; resid [B, H, W, Cout] (+ gate [Cout], default ones): out = resid + gate * y."""
    _req(x, torch.bfloat16, "x")
    _req(w2, torch.bfloat16, "w2")
    x = x.contiguous()
    B, Hi, Wi, Cc = x.shape
    Cout = w2.shape[0]
    if w2.shape[1] != 9 * Cc or not conv3x3_ok(Cc, Cout):
        raise ValueError(f"conv3x3: needs w2 [Cout, 9*C], C % 64 == 0, Cout % 128 == 0 (C={Cc}, w2={tuple(w2.shape)})")
    if upsample == -2:
        if Hi % 2 or Wi % 2:
            raise ValueError("conv3x3: the stride-2 mode needs even input dims")
        H, W = Hi // 2, Wi // 2
    else:
        H, W = Hi * upsample, Wi * upsample
    out = torch.empty((B, H, W, Cout), dtype=torch.bfloat16, device=x.device)
    if resid is not None:
        _req(resid, torch.bfloat16, "resid")
        resid = resid.contiguous()
        if gate is None:
            gate = torch.ones(Cout, dtype=torch.bfloat16, device=x.device)
    call("fluxmi_conv3x3", _p(x), _p(w2.contiguous()), _p(bias), _p(gate), _p(resid), _p(out), B, H, W, Cc, Cout, upsample, _stream())
    return out


CONV_DENSE_TILE = 16  # include/fluxmi.h FLUXMI_CONV_DENSE_TILE: the kernel's pixel tile edge


def _pixel_stride(t: torch.Tensor, name: str) -> int:
    """t: a [B, H, W, C] channel window of an NHWC pixel buffer -> its pixel stride in elements"""
    if t.ndim != 4 or t.stride(3) != 1:
        raise ValueError(f"conv3x3_dense: {name} must be a [B, H, W, C] view with channel stride 1, got {tuple(t.shape)} / {t.stride()}")
    B, H, W, _ = t.shape
    ld = t.stride(2) if W > 1 else (t.stride(1) if H > 1 else (t.stride(0) if B > 1 else t.shape[3] + (-t.shape[3]) % 8))
    ok = (W == 1 or t.stride(2) == ld) and (H == 1 or t.stride(1) == W * ld) and (B == 1 or t.stride(0) == H * W * ld)
    if not ok:
        raise ValueError(f"conv3x3_dense: {name} must address its pixels densely ([B][H][W] with ONE pixel stride), got strides {t.stride()}")
    return ld


def conv3x3_dense(x: torch.Tensor, w2: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, r1: Optional[torch.Tensor] = None,
                  a1: float = 1.0, r2: Optional[torch.Tensor] = None, a2: float = 1.0, slope: float = 0.2, act: bool = False,
                  upsample: int = 1) -> torch.Tensor:
    """The dense-block 3x3 convolution (fluxmi_conv3x3_dense; include/fluxmi.h has the arithmetic) on CHANNEL WINDOWS of NHWC bf16 pixel
    buffers: x [B, Hi, Wi, Cin] and out [B, H, W, Cout] are views such as buf[..., :Cin] and buf[..., Cin:Cin + Cout] (the same buffer is
    fine when the windows do not meet), r1 / r2 [B, H, W, Cout] likewise.  w2 [Cout32, 3, 3, Cin] (Cout32 = Cout rounded up to 32, extra
    rows zero), bias [Cout32] or None.  out = bf16(a2 * (a1 * lrelu(conv(x) + bias) + r1) + r2), each stage optional; H = upsample * Hi."""
    _req(x, torch.bfloat16, "x")
    _req(w2, torch.bfloat16, "w2")
    _req(out, torch.bfloat16, "out")
    ldx, ldo = _pixel_stride(x, "x"), _pixel_stride(out, "out")
    B, Hi, Wi, Cin = x.shape
    Bo, H, W, Cout = out.shape
    if upsample not in (1, 2) or (Bo, H, W) != (B, Hi * upsample, Wi * upsample):
        raise ValueError(f"conv3x3_dense: out {tuple(out.shape)} does not match x {tuple(x.shape)} at upsample={upsample}")
    c32 = (Cout + 31) // 32 * 32
    if not w2.is_contiguous() or w2.numel() != c32 * 9 * Cin or w2.shape[0] != c32:
        raise ValueError(f"conv3x3_dense: w2 must be contiguous [Cout32 = {c32}, 3, 3, Cin = {Cin}], got {tuple(w2.shape)}")
    if bias is not None:
        _req(bias, torch.bfloat16, "bias")
        if bias.numel() != c32 or not bias.is_contiguous():
            raise ValueError(f"conv3x3_dense: bias needs Cout32 = {c32} contiguous entries")
    ld_r = [0, 0]
    for i, r in enumerate((r1, r2)):
        if r is not None:
            _req(r, torch.bfloat16, f"r{i + 1}")
            if tuple(r.shape) != (B, H, W, Cout):
                raise ValueError(f"conv3x3_dense: r{i + 1} must be {(B, H, W, Cout)}, got {tuple(r.shape)}")
            ld_r[i] = _pixel_stride(r, f"r{i + 1}")
    call("fluxmi_conv3x3_dense", _p(x), ldx, Cin, _p(w2), _p(bias), _p(out), ldo, Cout, _p(r1), ld_r[0], float(a1), _p(r2), ld_r[1], float(a2),
         float(slope), int(bool(act)), upsample, B, H, W, _stream())
    return out


def im2col3x3(x: torch.Tensor, upsample: int = 1) -> torch.Tensor:
    """x [B, Hin, Win, C] bf16 -> patch matrix [B*H*W, 9*C], column order (dy, dx, c).  upsample = 1: H = Hin; 2: nearest 2x upsample
    first (H = 2*Hin); -2: stride-2 window with zero pad on the right/bottom only (H = Hin/2, the reference's Downsample)."""
    _req(x, torch.bfloat16, "x")
    x = x.contiguous()
    B, Hi, Wi, Cc = x.shape
    if upsample == -2:
        if Hi % 2 or Wi % 2:
            raise ValueError("im2col3x3: the stride-2 mode needs even input dims")
        H, W = Hi // 2, Wi // 2
    else:
        H, W = Hi * upsample, Wi * upsample
    col = torch.empty((B * H * W, 9 * Cc), dtype=torch.bfloat16, device=x.device)
    call("fluxmi_im2col3x3", _p(x), _p(col), B, H, W, Cc, upsample, _stream())
    return col


def groupnorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, swish: bool = True, eps: float = 1e-6) -> torch.Tensor:
    """x [B, P, C] bf16 (P pixels), 32 groups; fp32 statistics, one bf16 rounding at the end."""
    _req(x, torch.bfloat16, "x")
    x = x.contiguous()
    B, P, Cc = x.shape
    work = torch.empty((B * ((P + 511) // 512) + B) * 64, dtype=torch.float32, device=x.device)
    y = torch.empty_like(x)
    call("fluxmi_groupnorm", _p(x), _p(gamma), _p(beta), _p(y), _p(work), B, P, Cc, int(swish), float(eps), _stream())
    return y


def softmax_rows(S: torch.Tensor, scale: float) -> torch.Tensor:
    _req(S, torch.bfloat16, "S")
    S = S.contiguous()
    P = torch.empty_like(S)
    call("fluxmi_softmax_rows", _p(S), _p(P), S.shape[0], S.shape[1], S.stride(0), float(scale), _stream())
    return P


# ---- text-conditioning encoder pieces (bf16) ------------------------------------------------------------------------------
def row_norm(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, eps: float = 1e-6, rms: bool = True) -> torch.Tensor:
    """x [rows, D] bf16.  rms=True: T5LayerNorm (no mean / bias, weight applied after a bf16 rounding); else LayerNorm."""
    _req(x, torch.bfloat16, "x")
    if x.stride(-1) != 1:
        x = x.contiguous()
    y = torch.empty((x.shape[0], x.shape[1]), dtype=torch.bfloat16, device=x.device)
    call("fluxmi_row_norm", _p(x), _p(weight), _p(bias) if bias is not None else None, _p(y), x.shape[0], x.shape[1], x.stride(0), y.stride(0),
         float(eps), 0 if rms else 1, _stream())
    return y


def act_mul(x: torch.Tensor, gated: bool) -> torch.Tensor:
    """gated: x [rows, 2F] = [a | b] -> bf16(gelu_new(a)) * b [rows, F];  else quick_gelu(x)."""
    _req(x, torch.bfloat16, "x")
    x = x.contiguous()
    F_ = x.shape[1] // 2 if gated else x.shape[1]
    out = torch.empty((x.shape[0], F_), dtype=torch.bfloat16, device=x.device)
    call("fluxmi_act_mul", _p(x), _p(out), x.shape[0], F_, x.stride(0), out.stride(0), 0 if gated else 1, _stream())
    return out


def text_attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, L: int, heads: int, scale: float = 1.0, causal: bool = False,
                   rel_bias: Optional[torch.Tensor] = None, v_bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q, k [Lp, >= heads*64] (views with the same row stride), vt [heads*64, Lp] -> out [Lp, heads*64]; see include/fluxmi.h.
    Rows >= L of q and k and columns >= L of vt are padding the result does not depend on, but they must be FINITE (0 * inf is NaN in P V)."""
    _req(q, torch.bfloat16, "q")
    _req(k, torch.bfloat16, "k")
    _req(vt, torch.bfloat16, "vt")
    Lp = q.shape[0]
    if q.stride(0) != k.stride(0) or q.stride(1) != 1 or k.stride(1) != 1 or vt.stride(1) != 1:
        raise ValueError("text_attention: q and k must share the row stride; innermost strides must be 1")
    if out is None:
        out = torch.zeros((Lp, heads * 64), dtype=torch.bfloat16, device=q.device)
    if rel_bias is not None:
        _req(rel_bias, torch.float32, "rel_bias")
        rel_bias = rel_bias.contiguous()
    call("fluxmi_text_attention", _p(q), _p(k), q.stride(0), _p(vt), vt.stride(0), _p(out), out.stride(0),
         _p(rel_bias) if rel_bias is not None else None, rel_bias.shape[1] if rel_bias is not None else 0,
         _p(v_bias) if v_bias is not None else None, float(scale), int(causal), int(L), Lp, heads, _stream())
    return out


# ---- vision-encoder pieces (bf16) --------------------------------------------------------------------------------------------
def vision_attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, L: int, heads: int, head_dim: int, scale: float,
                     v_bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q, k [B, Lp, >= heads*head_dim] (views with the same strides), vt [B, heads*head_dim, Lp] -> out [B, Lp, heads*head_dim] (rows < L
    written): non-causal self-attention of B sequences in one launch, head width head_dim = 64 or 96 (zero-padded heads; see include/fluxmi.h)."""
    _req(q, torch.bfloat16, "q")
    _req(k, torch.bfloat16, "k")
    _req(vt, torch.bfloat16, "vt")
    B, Lp = q.shape[0], q.shape[1]
    if q.stride() != k.stride() or q.stride(2) != 1 or vt.stride(2) != 1 or tuple(k.shape[:2]) != (B, Lp):
        raise ValueError("vision_attention: q and k must share shape and strides; innermost strides must be 1")
    if vt.shape[0] != B or vt.shape[1] < heads * head_dim or vt.shape[2] < Lp:
        raise ValueError(f"vision_attention: vt must be [B, heads*head_dim, >= Lp], got {tuple(vt.shape)}")
    if q.shape[2] < heads * head_dim:
        raise ValueError(f"vision_attention: q must have >= heads*head_dim = {heads * head_dim} columns, got {q.shape[2]}")
    if out is None:
        out = torch.zeros((B, Lp, heads * head_dim), dtype=torch.bfloat16, device=q.device)
    if v_bias is not None:
        _req(v_bias, torch.bfloat16, "v_bias")
        if v_bias.numel() < heads * head_dim:
            raise ValueError("vision_attention: v_bias needs heads*head_dim entries")
    call("fluxmi_vision_attention", _p(q), _p(k), q.stride(1), q.stride(0), _p(vt), vt.stride(1), vt.stride(0), _p(out), out.stride(1),
         out.stride(0), _p(v_bias), float(scale), int(head_dim), int(L), Lp, int(heads), B, _stream())
    return out


def vae_attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, P: int, v_bias: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q, k [B, Pp, D] (views with the same strides, e.g. two column windows of one fused projection), vt [B, D, >= Pp] = V transposed ->
    out [B, P, D] = softmax(q k^T / sqrt D) v + v_bias: the autoencoder's single-head mid-block attention in ONE launch with no [P, P]
    matrix (fluxmi_vae_attention; include/fluxmi.h has the arithmetic).  D = 64 or 512; Pp = P rounded up to 64; rows >= P of q / k and
    columns >= P of vt are padding no output depends on (finite values).  Only rows < P of `out` are written."""
    _req(q, torch.bfloat16, "q")
    _req(k, torch.bfloat16, "k")
    _req(vt, torch.bfloat16, "vt")
    if q.ndim != 3 or k.ndim != 3 or vt.ndim != 3:
        raise ValueError("vae_attention: q, k [B, Pp, D] and vt [B, D, Pp] must be 3-d")
    B, Pp, D = q.shape
    P = int(P)
    if q.stride() != k.stride() or q.stride(2) != 1 or vt.stride(2) != 1 or tuple(k.shape) != (B, Pp, D):
        raise ValueError("vae_attention: q and k must share shape and strides; innermost strides must be 1")
    if D not in (64, 512):
        raise ValueError(f"vae_attention: head width D={D} must be 64 or 512")
    if P < 1 or Pp % 64 or Pp < P:
        raise ValueError(f"vae_attention: q / k must hold Pp rows, a multiple of 64 that is >= P (P={P}, Pp={Pp})")
    if vt.shape[0] != B or vt.shape[1] != D or vt.shape[2] < Pp:
        raise ValueError(f"vae_attention: vt must be [B, D, >= Pp] = [{B}, {D}, >= {Pp}], got {tuple(vt.shape)}")
    if out is None:
        out = torch.empty((B, P, D), dtype=torch.bfloat16, device=q.device)
    else:
        _req(out, torch.bfloat16, "out")
        if out.ndim != 3 or out.shape[0] != B or out.shape[1] < P or out.shape[2] != D or out.stride(2) != 1:
            raise ValueError(f"vae_attention: out must be [B, >= P, D] with innermost stride 1, got {tuple(out.shape)}")
    if v_bias is not None:
        _req(v_bias, torch.bfloat16, "v_bias")
        if v_bias.numel() != D or not v_bias.is_contiguous():
            raise ValueError(f"vae_attention: v_bias needs D = {D} contiguous entries")
    call("fluxmi_vae_attention", _p(q), _p(k), q.stride(1), q.stride(0), _p(vt), vt.stride(1), vt.stride(0), _p(out), out.stride(1),
         out.stride(0), _p(v_bias), D, P, Pp, B, _stream())
    return out


def patchify(pix: torch.Tensor, patch: int, grid: int, k_pad: int) -> torch.Tensor:
    """pix bf16 [B, C, H, W] -> patch rows [B*grid*grid, k_pad], column order (c, ky, kx), zero past C*patch*patch (fluxmi_patchify)."""
    _req(pix, torch.bfloat16, "pix")
    pix = pix.contiguous()
    B, Cc, H, W = pix.shape
    out = torch.empty((B * grid * grid, k_pad), dtype=torch.bfloat16, device=pix.device)
    call("fluxmi_patchify", _p(pix), _p(out), B, Cc, H, W, int(patch), int(grid), int(k_pad), _stream())
    return out


def add_scaled(x: torch.Tensor, r: torch.Tensor, scale) -> torch.Tensor:
    """In place x[b] = bf16(x[b] + bf16(r[b] * scale)) (fluxmi_add_scaled: the ControlNet residual hand-over).  x, r: bf16 [B, ...] whose
    samples are contiguous (the batch stride may exceed a sample's size); scale: a float or an fp32 device scalar, never rounded to bf16."""
    _req(x, torch.bfloat16, "x")
    _req(r, torch.bfloat16, "r")
    if x.shape != r.shape or x.ndim < 1:
        raise ValueError(f"add_scaled: x {tuple(x.shape)} vs r {tuple(r.shape)}")
    B = x.shape[0]
    n = x[0].numel() if B else 0
    for t in (x, r):
        if B and not t[0].is_contiguous():
            raise ValueError("add_scaled: the samples must be contiguous")
    s = scale if isinstance(scale, torch.Tensor) else torch.tensor([float(scale)], dtype=torch.float32, device=x.device)
    _req(s, torch.float32, "scale")
    xs = x.stride(0) if B > 1 else n
    rs = r.stride(0) if B > 1 else n
    _lib.call("fluxmi_add_scaled", _p(x), xs, _p(r), rs, _p(s), B, n, _stream())
    return x


def ip_attention(qkv: torch.Tensor, qn_scale: torch.Tensor, k_ip: torch.Tensor, v_ip: torch.Tensor, heads: int, nk: Optional[int] = None,
                 x: Optional[torch.Tensor] = None, scale=None) -> torch.Tensor:
    """The IP-Adapter term of a double block (fluxmi_ip_attention).  qkv: bf16 [B, rows, >= heads * 128] view of the image rows of a qkv GEMM
    output (q in the leading heads * 128 columns; row and batch strides are taken from the view); qn_scale: bf16 [128]; k_ip, v_ip: bf16
    [B, >= nk, heads * 128], of which rows [0, nk) are read (nk defaults to all).  x is None: returns o = bf16 [B, rows, heads * 128].  Else the
    fused form, in place: x = bf16(x + bf16(o * scale[b])), x a bf16 [B, rows, heads * 128] view (strided like qkv), scale a float or an fp32
    device tensor [B]."""
    for t, nm in ((qkv, "qkv"), (qn_scale, "qn_scale"), (k_ip, "k_ip"), (v_ip, "v_ip")):
        _req(t, torch.bfloat16, nm)
    hd = heads * 128
    if qkv.ndim != 3 or qkv.shape[-1] < hd or qkv.stride(-1) != 1 or qn_scale.numel() != 128 or not qn_scale.is_contiguous():
        raise ValueError(f"ip_attention: qkv {tuple(qkv.shape)} / qn_scale {tuple(qn_scale.shape)} for {heads} heads of 128")
    B, rows = qkv.shape[0], qkv.shape[1]
    nk = k_ip.shape[1] if nk is None else int(nk)
    if k_ip.shape != v_ip.shape or k_ip.ndim != 3 or k_ip.shape[0] != B or k_ip.shape[2] != hd or k_ip.shape[1] < nk or k_ip.stride() != v_ip.stride() \
            or k_ip.stride(2) != 1 or k_ip.stride(1) != hd:
        raise ValueError(f"ip_attention: k_ip {tuple(k_ip.shape)} / v_ip {tuple(v_ip.shape)} for B = {B}, nk = {nk}, {heads} heads")
    if x is None:
        out = torch.empty((B, rows, hd), dtype=torch.bfloat16, device=qkv.device)
        s, ss = None, 0
    else:
        out = _req(x, torch.bfloat16, "x")
        if out.shape != (B, rows, hd) or out.stride(-1) != 1:
            raise ValueError(f"ip_attention: x {tuple(out.shape)} vs [{B}, {rows}, {hd}]")
        s = scale if isinstance(scale, torch.Tensor) else torch.full((B,), float(scale), dtype=torch.float32, device=qkv.device)
        _req(s, torch.float32, "scale")
        if s.numel() != B:
            raise ValueError(f"ip_attention: {s.numel()} scales for {B} samples")
        ss = s.stride(0) if s.ndim else 0
    _lib.call("fluxmi_ip_attention", _p(qkv), qkv.stride(1), qkv.stride(0), _p(qn_scale), _p(k_ip), _p(v_ip), k_ip.stride(0), _p(out), out.stride(1),
              out.stride(0), _p(s), ss, B, rows, heads, nk, _stream())
    return out


# ---- guidance shaping of true CFG (fluxmi_guidance_moments / _combine; include/fluxmi.h) ---------------------------------------------------
GUIDANCE_MODES = {"cfg": 0, "apg": 1, "cfg_zero_star": 2}
GUIDANCE_CHUNK = 16384  # elements per workgroup of the moments pass


def guidance_params(s: float, mode="cfg", phi: float = 0.0, eta: float = 1.0, rho: float = 0.0, mu: float = 0.0, zero_init: int = 0):
    """The 8 floats {s, phi, eta, rho, mu, mode, zero_init, 0} the combine stage reads (a plain list; mode by name or number)."""
    m = GUIDANCE_MODES[mode] if isinstance(mode, str) else int(mode)
    return [float(s), float(phi), float(eta), float(rho), float(mu), float(m), float(zero_init), 0.0]


def _guidance_shape(pred: torch.Tensor, r: Optional[torch.Tensor]):
    _req(pred, torch.bfloat16, "pred")
    if pred.ndim < 2 or pred.shape[0] % 2 or not pred.is_contiguous():
        raise ValueError(f"guidance: pred {tuple(pred.shape)} must be contiguous [2B, ...]: prompt branches first, then the negative branches")
    B = pred.shape[0] // 2
    N = pred[0].numel()
    if r is not None:
        _req(r, torch.float32, "r")
        if r.numel() != B * N or not r.is_contiguous():
            raise ValueError(f"guidance: r {tuple(r.shape)} must be contiguous fp32 [{B}, {N}]")
    return B, N


def guidance_moments(pred: torch.Tensor, r: Optional[torch.Tensor] = None, part: Optional[torch.Tensor] = None) -> torch.Tensor:
    """part[b][g] = the nine fp32 sums (Sc, Su, Sr, cc, uu, rr, cu, cr, ur) over elements [16384 g, 16384 (g + 1)) of image b; pred bf16
    [2B, ...] (c = pred[b], u = pred[B + b]), r fp32 [B, N] or None (its sums are 0)."""
    B, N = _guidance_shape(pred, r)
    G = -(-N // GUIDANCE_CHUNK)
    if part is None:
        part = torch.empty((B, G, 9), dtype=torch.float32, device=pred.device)
    _req(part, torch.float32, "part")
    if part.numel() != B * G * 9 or not part.is_contiguous():
        raise ValueError(f"guidance_moments: part {tuple(part.shape)} must be contiguous fp32 [{B}, {G}, 9]")
    call("fluxmi_guidance_moments", _p(pred), _p(r), _p(part), B, N, _stream())
    return part


def guidance_combine(pred: torch.Tensor, part: torch.Tensor, params, r: Optional[torch.Tensor] = None, step=None, step_offset=None,
                     coef_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """In place: both halves of pred = bf16((alpha c + beta u) + gamma r) with the per-image coefficients of `params` (guidance_params, or an
    fp32 device tensor [8]) on the partial sums `part`; mu != 0 also advances r.  step / step_offset: ints or int32 device scalars (zero-init
    compares their sum with params[6]).  Returns coef_out, fp32 [B, 4] = {alpha, beta, gamma, f} per image."""
    B, N = _guidance_shape(pred, r)
    dev = pred.device
    prm = params if isinstance(params, torch.Tensor) else torch.tensor([float(v) for v in params], dtype=torch.float32, device=dev)
    _req(prm, torch.float32, "params")
    if prm.numel() != 8 or not prm.is_contiguous():
        raise ValueError("guidance_combine: params holds 8 floats {s, phi, eta, rho, mu, mode, zero_init, 0}")
    _req(part, torch.float32, "part")
    if part.numel() != B * (-(-N // GUIDANCE_CHUNK)) * 9 or not part.is_contiguous():
        raise ValueError(f"guidance_combine: part {tuple(part.shape)} is not guidance_moments' [B, ceil(N / {GUIDANCE_CHUNK}), 9]")
    ints = []
    for v in (step, step_offset):
        t = v if v is None or isinstance(v, torch.Tensor) else torch.tensor([int(v)], dtype=torch.int32, device=dev)
        ints.append(None if t is None else _req(t, torch.int32, "step"))
    if coef_out is None:
        coef_out = torch.empty((B, 4), dtype=torch.float32, device=dev)
    _req(coef_out, torch.float32, "coef_out")
    if coef_out.numel() != 4 * B or not coef_out.is_contiguous():
        raise ValueError(f"guidance_combine: coef_out {tuple(coef_out.shape)} must be contiguous fp32 [{B}, 4]")
    call("fluxmi_guidance_combine", _p(pred), _p(r), _p(part), _p(prm), _p(ints[0]), _p(ints[1]), _p(coef_out), B, N, _stream())
    return coef_out


def cfg_euler(img: torch.Tensor, pred: torch.Tensor, dt: float, scale: float) -> torch.Tensor:
    """In place, the guided Euler update (fluxmi_cfg_euler): img bf16 [2B, img_rows, c_in], pred bf16 [2B, pred_rows, c_out]; both halves of
    img get x + dt * (u + scale * (c - u)) on bf16 tensors, x read from the prompt half."""
    _req(img, torch.bfloat16, "img")
    _req(pred, torch.bfloat16, "pred")
    if img.ndim != 3 or pred.ndim != 3 or img.shape[0] != pred.shape[0] or img.shape[0] % 2 or not (img.is_contiguous() and pred.is_contiguous()):
        raise ValueError(f"cfg_euler: img {tuple(img.shape)} / pred {tuple(pred.shape)} must be contiguous [2B, rows, channels]")
    dts = torch.tensor([float(dt)], dtype=torch.float32, device=img.device)
    sc = torch.tensor([float(scale)], dtype=torch.float32, device=img.device)
    call("fluxmi_cfg_euler", _p(img), _p(pred), _p(dts), None, _p(sc), img.shape[0] // 2, img.shape[1], pred.shape[1], img.shape[2], pred.shape[2],
         _stream())
    return img


# ---- FlowEdit (fluxmi_flowedit_couple / _step; include/fluxmi.h, fluxmi/flowedit.py) ----------------------------------------------------------
def _flowedit_ids(ids, B: int, dev) -> torch.Tensor:
    """ids [B, 4] (a list of uint32 words, or a tensor) -> int32 device tensor holding the same 32-bit words"""
    t = ids if isinstance(ids, torch.Tensor) else torch.tensor([[int(w) for w in row] for row in ids], dtype=torch.int64).reshape(-1, 4)
    if tuple(t.shape) != (B, 4):
        raise ValueError(f"flowedit: ids {tuple(t.shape)}: expected [{B}, 4] uint32 words {{key_lo, key_hi, c2, c3}} per image")
    if t.dtype == torch.uint32:
        t = t.view(torch.int32)
    elif t.dtype != torch.int32:
        t = (((t.to(torch.int64) & 0xffffffff) + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)
    return t.to(dev).contiguous()


def flowedit_couple(z: torch.Tensor, x0: torch.Tensor, t: float, ids, eval_index: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """FlowEdit's coupling alone (fluxmi_flowedit_couple): z, x0 bf16 [B, rows, C] -> out bf16 [2B, rows, C] with zs = (1 - t) * x0 + t * n in
    the first half and zt = z + zs - x0 in the second, on bf16 tensors, n the Philox normals of (ids[b], eval_index) rounded to bf16.  1 - t is
    subtracted here, in double."""
    _req(z, torch.bfloat16, "z")
    _req(x0, torch.bfloat16, "x0")
    if z.ndim != 3 or z.shape != x0.shape or not (z.is_contiguous() and x0.is_contiguous()):
        raise ValueError(f"flowedit_couple: z {tuple(z.shape)} / x0 {tuple(x0.shape)} must be contiguous [B, rows, channels] of one shape")
    B, R, Cc = z.shape
    d_ids = _flowedit_ids(ids, B, z.device)
    if out is None:
        out = torch.empty((2 * B, R, Cc), dtype=torch.bfloat16, device=z.device)
    _req(out, torch.bfloat16, "out")
    if tuple(out.shape) != (2 * B, R, Cc) or not out.is_contiguous():
        raise ValueError(f"flowedit_couple: out {tuple(out.shape)} must be contiguous [{2 * B}, {R}, {Cc}]")
    call("fluxmi_flowedit_couple", _p(out), _p(z), _p(x0), float(t), float(1.0 - float(t)), _p(d_ids), int(eval_index), B, R, R, Cc, Cc, _stream())
    return out


def flowedit_step(img: torch.Tensor, pred: torch.Tensor, z: torch.Tensor, x0: torch.Tensor, coef: torch.Tensor, ctl: torch.Tensor, ids,
                  acc: Optional[torch.Tensor] = None, step: Optional[torch.Tensor] = None, eval_offset: Optional[torch.Tensor] = None) -> torch.Tensor:
    """In place, FlowEdit's update and the next coupling (fluxmi_flowedit_step): img / pred bf16 [2B, rows, C], z / x0 bf16 [B, rows, C], coef
    fp32 [n, 4] and ctl int32 [n, 2] on the device, `step` / `eval_offset` int32 device scalars (None = 0), acc fp32 [B, rows, C] or None."""
    for name, t_ in (("img", img), ("pred", pred), ("z", z), ("x0", x0)):
        _req(t_, torch.bfloat16, name)
    _req(coef, torch.float32, "coef")
    _req(ctl, torch.int32, "ctl")
    if acc is not None:
        _req(acc, torch.float32, "acc")
    B, R, Cc = z.shape
    if tuple(img.shape) != (2 * B, R, Cc) or pred.shape != img.shape or x0.shape != z.shape or (acc is not None and acc.shape != z.shape) or \
            not all(t_.is_contiguous() for t_ in (img, pred, z, x0, coef, ctl) + ((acc,) if acc is not None else ())):
        raise ValueError(f"flowedit_step: img {tuple(img.shape)} / pred {tuple(pred.shape)} [2B, rows, C] and z {tuple(z.shape)} / x0 / acc [B, rows, C], contiguous")
    d_ids = _flowedit_ids(ids, B, z.device)
    call("fluxmi_flowedit_step", _p(img), _p(pred), _p(z), _p(acc), _p(x0), _p(coef), _p(ctl), _p(step), _p(d_ids), _p(eval_offset), B, R, R, Cc, Cc,
         _stream())
    return z


# ---- tiled generation (fluxmi_window_gather / _step; include/fluxmi.h, fluxmi/windows.py) ---------------------------------------------------
def _window_shapes(who: str, canvas: torch.Tensor, img: torch.Tensor, row0, col0, h: int, w: int, guided: bool):
    """canvas bf16 [N, Hc, Wc, C], img bf16 [S or 2S, h * w, C] with S = N * ny * nx, contiguous -> (N, Hc, Wc, ny, nx, C).  What the tables
    hold, and C % 8, is the library's to refuse."""
    _req(canvas, torch.bfloat16, "canvas")
    _req(img, torch.bfloat16, "img")
    for name, t in (("row0", row0), ("col0", col0)):
        if t is not None:
            _req(t, torch.int32, name)
    if canvas.ndim != 4 or img.ndim != 3 or not (canvas.is_contiguous() and img.is_contiguous()):
        raise ValueError(f"{who}: canvas {tuple(canvas.shape)} must be contiguous [N, Hc, Wc, C] and img {tuple(img.shape)} contiguous [S, h * w, C]")
    N, Hc, Wc, Cc = canvas.shape
    ny, nx = (1 if row0 is None else row0.numel()), (1 if col0 is None else col0.numel())
    S = N * ny * nx * (2 if guided else 1)
    if tuple(img.shape) != (S, int(h) * int(w), Cc):
        raise ValueError(f"{who}: img {tuple(img.shape)}: expected [{S}, {int(h) * int(w)}, {Cc}] ({N} images x {ny} x {nx} windows"
                         f"{', both branches' if guided else ''})")
    return N, Hc, Wc, ny, nx, Cc


def window_gather(canvas: torch.Tensor, img: torch.Tensor, row0: torch.Tensor, col0: torch.Tensor, h: int, w: int, guided: bool = False) -> torch.Tensor:
    """Fills the stream from the canvas (fluxmi_window_gather): canvas bf16 [N, Hc, Wc, C]; img bf16 [S, h * w, C], S = N * ny * nx, sample
    (n * ny + a) * nx + b window (a, b) of image n at canvas token (row0[a], col0[b]); `guided`: img holds 2S samples and both halves are
    filled.  row0 / col0: int32 device tensors.  Returns img."""
    N, Hc, Wc, ny, nx, Cc = _window_shapes("window_gather", canvas, img, row0, col0, h, w, guided)
    call("fluxmi_window_gather", _p(canvas), _p(img), _p(row0), _p(col0), N, Hc, Wc, int(h), int(w), ny, nx, Cc, int(bool(guided)), _stream())
    return img


def window_step(canvas: torch.Tensor, img: torch.Tensor, pred: torch.Tensor, dts: torch.Tensor, row0: torch.Tensor, col0: torch.Tensor,
                Ny: torch.Tensor, Nx: torch.Tensor, h: int, w: int, step: Optional[torch.Tensor] = None,
                scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """In place, the windowed update (fluxmi_window_step): the canvas moves by dts[*step] times the blend of the windows' predictions
    (`scale`, an fp32 device scalar: of their guided predictions, pred / img then hold 2S samples) and every window of img is rebuilt from
    it.  dts fp32, `step` an int32 device scalar (None = 0), Ny fp32 [ny, Hc] / Nx fp32 [nx, Wc] (fluxmi.windows.window_weights) on the
    device.  Returns the canvas."""
    guided = scale is not None
    N, Hc, Wc, ny, nx, Cc = _window_shapes("window_step", canvas, img, row0, col0, h, w, guided)
    _req(pred, torch.bfloat16, "pred")
    _req(dts, torch.float32, "dts")
    if pred.shape != img.shape or not pred.is_contiguous():
        raise ValueError(f"window_step: pred {tuple(pred.shape)} must be contiguous like img {tuple(img.shape)}")
    for name, t, want in (("Ny", Ny, (ny, Hc)), ("Nx", Nx, (nx, Wc))):
        if t is not None:
            _req(t, torch.float32, name)
            if tuple(t.shape) != want or not t.is_contiguous():
                raise ValueError(f"window_step: {name} {tuple(t.shape)} must be contiguous fp32 {list(want)}")
    if step is not None:
        _req(step, torch.int32, "step")
    if guided:
        _req(scale, torch.float32, "scale")
    call("fluxmi_window_step", _p(canvas), _p(img), _p(pred), _p(dts), _p(step), _p(scale), _p(row0), _p(col0), _p(Ny), _p(Nx), N, Hc, Wc, int(h),
         int(w), ny, nx, Cc, _stream())
    return canvas


# ---- latent preview (fluxmi_latent_preview; include/fluxmi.h) ---------------------------------------------------------------------------
def preview_proj(factors, bias=None) -> list:
    """The 51 floats the kernel reads: M[16][3] row-major, then bias[3] (zeros when None)."""
    m = [[float(v) for v in row] for row in factors]
    b = [0.0, 0.0, 0.0] if bias is None else [float(v) for v in bias]
    if len(m) != 16 or any(len(r) != 3 for r in m) or len(b) != 3:
        raise ValueError("preview_proj: factors [16][3] and bias [3]")
    return [v for r in m for v in r] + b


def latent_preview(x: torch.Tensor, pred: torch.Tensor, t, proj, grid, scale=None, step=None, ctl=None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The denoised estimate x - t v of one evaluation projected to RGB (fluxmi_latent_preview): x bf16 [B (2B guided), img_rows, c_in],
    pred bf16 [B (2B guided), pred_rows, 64], `grid` = (h, w) tokens, proj = the 51 floats (a list or an fp32 device tensor).  `t`: a float,
    or an fp32 device table indexed by `step` (an int32 device scalar; None = entry 0).  `scale` (a float or an fp32 device scalar) selects
    the guided form.  `ctl` = (every, eval_offset) or an int32 device tensor [2]; None = (1, 0): every evaluation, slot = step % PREVIEW_SLOTS.
    Returns `out`, uint8 [PREVIEW_SLOTS, B, 2 h, 2 w, 3]: only the slot the launch selects is written."""
    _req(x, torch.bfloat16, "x")
    _req(pred, torch.bfloat16, "pred")
    if x.ndim != 3 or pred.ndim != 3 or x.shape[0] != pred.shape[0] or not (x.is_contiguous() and pred.is_contiguous()):
        raise ValueError(f"latent_preview: x {tuple(x.shape)} / pred {tuple(pred.shape)} must be contiguous [B, rows, channels] of one batch")
    dev = x.device
    guided = scale is not None
    if guided and x.shape[0] % 2:
        raise ValueError("latent_preview: a guided call takes [2B, ...]: prompt branches first, then the negative branches")
    B = x.shape[0] // 2 if guided else x.shape[0]
    h, w = int(grid[0]), int(grid[1])
    f32t = lambda v, name: _req(v if isinstance(v, torch.Tensor) else torch.tensor([float(u) for u in (v if isinstance(v, (list, tuple)) else [v])],
                                                                                    dtype=torch.float32, device=dev), torch.float32, name)
    ts, prj = f32t(t, "t"), f32t(proj, "proj")
    if prj.numel() != 51 or not prj.is_contiguous():
        raise ValueError("latent_preview: proj holds 51 floats: M[16][3], then bias[3]")
    sc = f32t(scale, "scale") if guided else None
    st = None if step is None else _req(step if isinstance(step, torch.Tensor) else torch.tensor([int(step)], dtype=torch.int32, device=dev),
                                        torch.int32, "step")
    ct = None if ctl is None else _req(ctl if isinstance(ctl, torch.Tensor) else torch.tensor([int(v) for v in ctl], dtype=torch.int32, device=dev),
                                       torch.int32, "ctl")
    if ct is not None and ct.numel() != 2:
        raise ValueError("latent_preview: ctl holds {every, eval_offset}")
    if out is None:
        out = torch.zeros((_lib.PREVIEW_SLOTS, B, 2 * h, 2 * w, 3), dtype=torch.uint8, device=dev)
    _req(out, torch.uint8, "out")
    if out.numel() != _lib.PREVIEW_SLOTS * B * 4 * h * w * 3 or not out.is_contiguous():
        raise ValueError(f"latent_preview: out {tuple(out.shape)} must be contiguous uint8 [{_lib.PREVIEW_SLOTS}, {B}, {2 * h}, {2 * w}, 3]")
    call("fluxmi_latent_preview", _p(x), _p(pred), _p(ts), _p(st), _p(sc), _p(prj), _p(ct), _p(out), B, x.shape[1], pred.shape[1], x.shape[2], pred.shape[2], h, w, _stream())
    return out


# ---- control-map preprocessors (csrc/preprocess.hip; include/fluxmi.h has the arithmetic) ----------------------------------------------
CANNY_TILE = 32          # FLUXMI_CANNY_TILE: the pixel tile edge of the classify and the hysteresis kernel
CANNY_ROUND_GROUP = 4    # FLUXMI_CANNY_ROUND_GROUP: hysteresis rounds launched per flag read-back
BLUR_MAX_RADIUS = 64     # FLUXMI_BLUR_MAX_RADIUS


def _u8_image(t: torch.Tensor, who: str, name: str, channels: int):
    """t: uint8 [B, H, W, channels] (or [B, H, W] for channels == 1), pixels and channels adjacent, any row / image stride that keeps rows
    apart (a window of a larger buffer is fine) -> (B, H, W, row stride, image stride) in bytes"""
    _req(t, torch.uint8, f"{who}: {name}")
    shape = tuple(t.shape) + (1,) if t.ndim == 3 and channels == 1 else tuple(t.shape)
    strides = tuple(t.stride()) + (1,) if t.ndim == 3 and channels == 1 else tuple(t.stride())
    if len(shape) != 4 or shape[3] != channels or min(shape) < 1:
        want = f"[B, H, W, {channels}]" + (" or [B, H, W]" if channels == 1 else "")
        raise ValueError(f"{who}: {name} must be uint8 {want} with B, H, W >= 1, got {tuple(t.shape)}")
    B, H, W, C = shape
    ld = strides[1] if H > 1 else W * C
    bs = strides[0] if B > 1 else H * ld
    if (C > 1 and strides[3] != 1) or (W > 1 and strides[2] != C) or ld < W * C or bs < H * ld:
        raise ValueError(f"{who}: {name} must keep channels and pixels adjacent, rows >= W * C = {W * C} bytes apart and images >= H rows "
                         f"apart, got strides {tuple(t.stride())} for shape {tuple(t.shape)}")
    return B, H, W, ld, bs


def _u8_out(out: Optional[torch.Tensor], shape, like: torch.Tensor, who: str, name: str, channels: int):
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=like.device)
    geo = _u8_image(out, who, name, channels)
    if out.device != like.device or geo[:3] != tuple(shape[:3]):
        raise ValueError(f"{who}: {name} {tuple(out.shape)} on {out.device} does not match the input's {tuple(shape)} on {like.device}")
    return out, geo[3], geo[4]


def canny_thresholds(low, high):
    """Canny's two thresholds as the kernel takes them: integers >= 0 (bools and fractions are refused by name), in either order."""
    for name, v in (("low", low), ("high", high)):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** 31:
            raise ValueError(f"canny: {name}={v!r}: expected an integer in [0, 2^31)")
    return int(low), int(high)


def blur_radius(sigma) -> int:
    """ceil(3 sigma) with sigma rounded to fp32 first, as fluxmi_gaussian_blur computes it; refuses a sigma whose radius is outside
    1..BLUR_MAX_RADIUS"""
    import math

    try:
        s = float(torch.tensor(float(sigma), dtype=torch.float32))
    except (TypeError, ValueError):
        raise ValueError(f"gaussian_blur: sigma={sigma!r}: expected a number (the radius is ceil(3 sigma))") from None
    r = math.ceil(3.0 * s) if math.isfinite(s) and s > 0 else 0
    if isinstance(sigma, bool) or not 1 <= r <= BLUR_MAX_RADIUS:
        raise ValueError(f"gaussian_blur: sigma={sigma!r}: the radius ceil(3 sigma) must lie in 1..{BLUR_MAX_RADIUS}")
    return r


def rgb_to_gray(rgb: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """rgb uint8 [B, H, W, 3] -> uint8 [B, H, W]: L = (19595 R + 38470 G + 7471 B + 32768) >> 16, PIL's convert("L") bit for bit"""
    B, H, W, ld, bs = _u8_image(rgb, "rgb_to_gray", "rgb", 3)
    out, old, obs = _u8_out(out, (B, H, W), rgb, "rgb_to_gray", "out", 1)
    call("fluxmi_rgb_to_gray", _p(rgb), ld, bs, _p(out), old, obs, B, H, W, _stream())
    return out


def canny_classify(rgb: torch.Tensor, low: int, high: int, l2: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The first half of Canny (fluxmi_canny_classify): rgb uint8 [B, H, W, 3] -> state uint8 [B, H, W], 0 = no edge, 1 = weak (kept by
    non-maximum suppression, above min(low, high)), 2 = strong (above max(low, high)).  l2: squared-gradient magnitudes against squared thresholds."""
    low, high = canny_thresholds(low, high)
    B, H, W, ld, bs = _u8_image(rgb, "canny_classify", "rgb", 3)
    out, old, obs = _u8_out(out, (B, H, W), rgb, "canny_classify", "out", 1)
    call("fluxmi_canny_classify", _p(rgb), ld, bs, _p(out), old, obs, B, H, W, low, high, int(bool(l2)), _stream())
    return out


def canny_hysteresis(state: torch.Tensor, out: Optional[torch.Tensor] = None):
    """The second half (fluxmi_canny_hysteresis): state uint8 [B, H, W] of 0 / 1 / 2 -> (edges, rounds); edges uint8 [B, H, W] is 255 on every
    strong pixel and every weak pixel 8-connected to one through weak pixels, 0 elsewhere; `rounds` = kernel rounds run, the last of which
    changed nothing.  `state` is left as it is (the rounds run on a copy).  Reads flags back: synchronises the current stream."""
    B, H, W, _, _ = _u8_image(state, "canny_hysteresis", "state", 1)
    out, old, obs = _u8_out(out, (B, H, W), state, "canny_hysteresis", "out", 1)
    work = state.reshape(B, H, W).clone(memory_format=torch.contiguous_format)
    flags = torch.zeros(CANNY_ROUND_GROUP, dtype=torch.int32, device=state.device)
    rounds = C.c_int(0)
    call("fluxmi_canny_hysteresis", _p(work), W, H * W, _p(out), old, obs, _p(flags), B, H, W, C.byref(rounds), _stream())
    return out, rounds.value


def canny(rgb: torch.Tensor, low: int, high: int, l2: bool = False, out: Optional[torch.Tensor] = None, return_rounds: bool = False):
    """The Canny edge detector (fluxmi_canny = classify + hysteresis): rgb uint8 [B, H, W, 3] -> edges uint8 [B, H, W] of 0 / 255.  Integer
    arithmetic throughout; include/fluxmi.h is the definition (parity with an OpenCV binary is not pinned).  Synchronises the current stream."""
    low, high = canny_thresholds(low, high)
    B, H, W, ld, bs = _u8_image(rgb, "canny", "rgb", 3)
    out, old, obs = _u8_out(out, (B, H, W), rgb, "canny", "out", 1)
    nbytes = B * H * ((W + 3) // 4 * 4) + 4 * CANNY_ROUND_GROUP  # FLUXMI_CANNY_WORK_BYTES
    work = torch.empty(nbytes, dtype=torch.uint8, device=rgb.device)
    rounds = C.c_int(0)
    call("fluxmi_canny", _p(rgb), ld, bs, _p(out), old, obs, _p(work), nbytes, B, H, W, low, high, int(bool(l2)), C.byref(rounds), _stream())
    return (out, rounds.value) if return_rounds else out


def gaussian_blur(img: torch.Tensor, sigma: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Separable Gaussian blur (fluxmi_gaussian_blur) of img uint8 [B, H, W, C], C in {1, 3} ([B, H, W] counts as C = 1): radius
    ceil(3 sigma) in 1..64, replicated border, fp32 accumulation over an fp32 intermediate, one rounding at the store."""
    blur_radius(sigma)
    ch = 1 if img.ndim == 3 else img.shape[-1]
    if ch not in (1, 3):
        raise ValueError(f"gaussian_blur: img {tuple(img.shape)}: expected 1 or 3 channels")
    B, H, W, ld, bs = _u8_image(img, "gaussian_blur", "img", ch)
    out, old, obs = _u8_out(out, tuple(img.shape), img, "gaussian_blur", "out", ch)
    if out.data_ptr() == img.data_ptr():
        raise ValueError("gaussian_blur: out must not be img")
    nbytes = B * H * ((W * ch + 3) // 4 * 4) * 4  # FLUXMI_BLUR_WORK_BYTES
    work = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
    call("fluxmi_gaussian_blur", _p(img), ld, bs, _p(out), old, obs, _p(work), nbytes, B, H, W, ch, float(sigma), _stream())
    return out


# ---- baseline JPEG encoder (csrc/jpeg.hip, csrc/jpeg_host.cpp; include/fluxmi.h has the definition) -----------------------------------------
JPEG_SUBSAMPLING = {"4:2:0": 0, "4:4:4": 1}             # FLUXMI_JPEG_420 / FLUXMI_JPEG_444
JPEG_DEFAULT_RESTART = {"4:2:0": 4, "4:4:4": 8}         # FLUXMI_JPEG_RESTART_420 / _444: MCUs per interval, 24 blocks either way
JPEG_MAX_DIM = 65535


def jpeg_params(B: int, H: int, W: int, quality=99, subsampling="4:2:0", restart_interval=None):
    """every refusal of a JPEG request that needs no device, by name -> (quality, FLUXMI_JPEG_* code, MCUs per interval); restart_interval
    None = JPEG_DEFAULT_RESTART[subsampling], 0 = no restart markers (one workgroup codes the whole image: slow)"""
    if subsampling not in JPEG_SUBSAMPLING:
        raise ValueError(f"jpeg_encode: subsampling={subsampling!r}: expected one of {tuple(JPEG_SUBSAMPLING)}")
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f"jpeg_encode: quality={quality!r}: expected an integer in 1..100")
    if restart_interval is None:
        restart_interval = JPEG_DEFAULT_RESTART[subsampling]
    if isinstance(restart_interval, bool) or not isinstance(restart_interval, int) or not 0 <= restart_interval <= 65535:
        raise ValueError(f"jpeg_encode: restart_interval={restart_interval!r}: expected an integer in 0..65535 (MCUs per interval; 0 = no "
                         f"restart markers, None = {JPEG_DEFAULT_RESTART[subsampling]})")
    if W > JPEG_MAX_DIM or B * H > JPEG_MAX_DIM:
        raise ValueError(f"jpeg_encode: a JPEG holds at most {JPEG_MAX_DIM} x {JPEG_MAX_DIM} pixels: width {W}, height {B} x {H} = {B * H} "
                         f"(a batch is one image, stacked vertically)")
    return quality, JPEG_SUBSAMPLING[subsampling], restart_interval


def jpeg_workspace_bytes(B: int, H: int, W: int, subsampling="4:2:0", restart_interval=None):
    """(bytes of `work`, bytes of an `out` no stream can exceed) for jpeg_encode_into (fluxmi_jpeg_workspace_bytes)"""
    _, ss, R = jpeg_params(B, H, W, 99, subsampling, restart_interval)
    work, cap = C.c_longlong(0), C.c_longlong(0)
    call("fluxmi_jpeg_workspace_bytes", B, H, W, ss, R, C.byref(work), C.byref(cap))
    return work.value, cap.value


def jpeg_header(B: int, H: int, W: int, quality=99, subsampling="4:2:0", restart_interval=None) -> bytes:
    """the header (SOI .. SOS) of the file jpeg_encode writes for such an input, from the host (fluxmi_jpeg_header)"""
    q, ss, R = jpeg_params(B, H, W, quality, subsampling, restart_interval)
    buf, n = C.create_string_buffer(1024), C.c_longlong(0)
    call("fluxmi_jpeg_header", B, H, W, q, ss, R, buf, 1024, C.byref(n))
    return buf.raw[:n.value]


def _jpeg_run(px: torch.Tensor, work: torch.Tensor, out: torch.Tensor, quality, subsampling, restart_interval) -> int:
    """the launches and the 8-byte read-back -> the stream's length, which exceeds out.numel() when the stream did not fit (`out` then holds
    its first bytes and nothing beyond `out` was written)"""
    B, H, W, ld, bs = _u8_image(px, "jpeg_encode", "px", 3)
    q, ss, R = jpeg_params(B, H, W, quality, subsampling, restart_interval)
    for name, t in (("work", work), ("out", out)):
        _req(t, torch.uint8, f"jpeg_encode: {name}")
        if t.ndim != 1 or not t.is_contiguous() or t.device != px.device:
            raise ValueError(f"jpeg_encode: {name} must be a flat contiguous uint8 buffer on {px.device}")
    need, _ = jpeg_workspace_bytes(B, H, W, subsampling, R)
    if work.numel() < need:
        raise ValueError(f"jpeg_encode: work holds {work.numel()} bytes, jpeg_workspace_bytes gives {need}")
    n_dev = torch.zeros(1, dtype=torch.int64, device=px.device)
    call("fluxmi_jpeg_encode", _p(px), ld, bs, B, H, W, q, ss, R, _p(work), _p(out), out.numel(), _p(n_dev), _stream())
    n = C.c_longlong(0)
    rc = _lib.lib.fluxmi_jpeg_finish(_p(n_dev), out.numel(), C.byref(n), _stream())
    if rc != 0 and n.value <= out.numel():  # anything but "did not fit"
        _lib.check(rc)
    return n.value


def jpeg_encode_into(px: torch.Tensor, work: torch.Tensor, out: torch.Tensor, quality=99, subsampling="4:2:0", restart_interval=None) -> int:
    """px uint8 [B, H, W, 3] on the device (any row / image stride, as _u8_image takes them) -> the JPEG file in out[:n], n returned.  work
    (256-byte aligned) and out are flat uint8 device buffers; work holds jpeg_workspace_bytes(...)[0] bytes, out any number: a stream that
    does not fit is refused by name (RuntimeError) and nothing beyond out is written.  One small device-to-host copy (the length)."""
    n = _jpeg_run(px, work, out, quality, subsampling, restart_interval)
    if n > out.numel():
        raise RuntimeError("fluxmi: " + _lib.lib.fluxmi_last_error().decode("utf-8", "replace"))
    return n


def jpeg_encode(px: torch.Tensor, quality: int = 99, subsampling: str = "4:2:0", restart_interval: Optional[int] = None) -> bytes:
    """px uint8 [B, H, W, 3] on the device -> the bytes of a baseline JFIF file (fluxmi_jpeg_encode; include/fluxmi.h is the definition,
    libjpeg's integer pipeline at its defaults).  A batch is ONE image of height B * H.  Two device-to-host copies: the length, then exactly
    that many bytes.  Synchronises the current stream."""
    B, H, W, _, _ = _u8_image(px, "jpeg_encode", "px", 3)
    nwork, cap = jpeg_workspace_bytes(B, H, W, subsampling, restart_interval)
    work = torch.empty(nwork, dtype=torch.uint8, device=px.device)
    # `cap` is the worst case (every coefficient at its longest code, every byte stuffed): 9.75 or 19.5 bytes per pixel.  The raw size is tried
    # first -- only noise at the highest qualities exceeds it -- and a stream that did not fit is coded again into the worst case
    first = min(cap, 1024 + 3 * B * H * W)
    out = torch.empty(first, dtype=torch.uint8, device=px.device)
    n = _jpeg_run(px, work, out, quality, subsampling, restart_interval)
    if n > first:
        out = torch.empty(cap, dtype=torch.uint8, device=px.device)
        n = jpeg_encode_into(px, work, out, quality, subsampling, restart_interval)
    host = torch.empty(n, dtype=torch.uint8, pin_memory=True)  # torch caches pinned blocks: no allocation once warm
    host.copy_(out[:n], non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return host.numpy().tobytes()


# ---- depth estimator pieces (csrc/depth.hip; NHWC bf16 maps behind one pixel stride) ------------------------------------------------------
UNARY_KINDS = {"gelu": 0, "relu": 1}            # FLUXMI_UNARY_GELU_ERF / FLUXMI_UNARY_RELU
DEPTH_NORMALIZE = {"minmax": 0, "raw": 1}       # FLUXMI_DEPTH_MINMAX / FLUXMI_DEPTH_RAW


def unary(x: torch.Tensor, kind: str, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = bf16(f(x)) elementwise in fp32 with one rounding (fluxmi_unary): kind "gelu" = the exact GELU 0.5 x (1 + erf(x / sqrt 2)),
    "relu".  x bf16 [..., cols] whose leading dims collapse to rows of ONE stride (a column window of a wider buffer is fine), any cols;
    `out`: a tensor of x's shape under the same rule (default: a new dense one; may be x)."""
    _req(x, torch.bfloat16, "x")
    if kind not in UNARY_KINDS:
        raise ValueError(f"unary: kind={kind!r}: expected one of {tuple(UNARY_KINDS)}")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    _req(out, torch.bfloat16, "out")
    if tuple(out.shape) != tuple(x.shape):
        raise ValueError(f"unary: out {tuple(out.shape)} does not match x {tuple(x.shape)}")
    if x.numel() == 0:
        return out

    def rows_of(t, name):
        cols = t.shape[-1]
        if t.ndim < 1 or (cols > 1 and t.stride(-1) != 1):
            raise ValueError(f"unary: {name} must have unit stride along its last dim, got strides {t.stride()}")
        lead = [(n, s) for n, s in zip(t.shape[:-1], t.stride()[:-1]) if n > 1]
        ld = lead[-1][1] if lead else cols
        want = ld
        for n, s in reversed(lead):
            if s != want:
                raise ValueError(f"unary: the rows of {name} must lie at ONE stride, got shape {tuple(t.shape)} / strides {t.stride()}")
            want *= n
        return ld

    ldx, ldo = rows_of(x, "x"), rows_of(out, "out")
    cols = x.shape[-1]
    call("fluxmi_unary", _p(x), _p(out), x.numel() // cols, cols, ldx, ldo, UNARY_KINDS[kind], _stream())
    return out


def _depth_pixels(t: torch.Tensor, who: str, name: str):
    """t: a bf16 [B, H, W, C] channel window of an NHWC pixel buffer with ONE pixel stride -> that stride in elements"""
    _req(t, torch.bfloat16, f"{who}: {name}")
    if t.ndim != 4 or min(t.shape) < 1 or t.stride(3) != 1:
        raise ValueError(f"{who}: {name} must be a bf16 [B, H, W, C] view with channel stride 1, got {tuple(t.shape)} / {t.stride()}")
    B, H, W, Cc = t.shape
    ld = t.stride(2) if W > 1 else (t.stride(1) if H > 1 else (t.stride(0) if B > 1 else Cc + (-Cc) % 8))
    if not ((W == 1 or t.stride(2) == ld) and (H == 1 or t.stride(1) == W * ld) and (B == 1 or t.stride(0) == H * W * ld)):
        raise ValueError(f"{who}: {name} must address its pixels densely ([B][H][W] with ONE pixel stride), got strides {t.stride()}")
    return ld


def resize_bilinear(x: torch.Tensor, size, add: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x bf16 [B, Hi, Wi, C] (NHWC, or a channel window of a wider pixel buffer) -> [B, Ho, Wo, C], size = (Ho, Wo): the bilinear resize
    with align_corners=True as torch computes it (fluxmi_resize_bilinear; include/fluxmi.h has the arithmetic), any sizes >= 1, C % 8 == 0.
    `add` [B, Ho, Wo, C]: out = bf16(bf16(resize(x)) + add).  `out`: a [B, Ho, Wo, C] view to write (default: a new dense tensor)."""
    ldx = _depth_pixels(x, "resize_bilinear", "x")
    B, Hi, Wi, Cc = x.shape
    Ho, Wo = int(size[0]), int(size[1])
    if Ho < 1 or Wo < 1 or Cc % 8:
        raise ValueError(f"resize_bilinear: size {tuple(size)} must be >= 1 x 1 and C = {Cc} a multiple of 8")
    if out is None:
        out = torch.empty((B, Ho, Wo, Cc), dtype=torch.bfloat16, device=x.device)
    if tuple(out.shape) != (B, Ho, Wo, Cc):
        raise ValueError(f"resize_bilinear: out {tuple(out.shape)} does not match {(B, Ho, Wo, Cc)}")
    ldo = _depth_pixels(out, "resize_bilinear", "out")
    lda = 0
    if add is not None:
        if tuple(add.shape) != (B, Ho, Wo, Cc):
            raise ValueError(f"resize_bilinear: add {tuple(add.shape)} does not match {(B, Ho, Wo, Cc)}")
        lda = _depth_pixels(add, "resize_bilinear", "add")
    call("fluxmi_resize_bilinear", _p(x), ldx, _p(out), ldo, _p(add), lda, B, Hi, Wi, Ho, Wo, Cc, _stream())
    return out


def patchify_rect(pix: torch.Tensor, patch: int, grid_h: int, grid_w: int, k_pad: int) -> torch.Tensor:
    """pix bf16 [B, C, H, W] -> patch rows [B*grid_h*grid_w, k_pad], column order (c, ky, kx), zero past C*patch*patch (fluxmi_patchify_rect)."""
    _req(pix, torch.bfloat16, "pix")
    pix = pix.contiguous()
    B, Cc, H, W = pix.shape
    out = torch.empty((B * grid_h * grid_w, k_pad), dtype=torch.bfloat16, device=pix.device)
    call("fluxmi_patchify_rect", _p(pix), _p(out), B, Cc, H, W, int(patch), int(grid_h), int(grid_w), int(k_pad), _stream())
    return out


def conv3x3_s2_hw(Hi: int, Wi: int):
    """the output grid of Conv2d(kernel 3, stride 2, padding 1)"""
    return (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1


def im2col3x3_s2(x: torch.Tensor) -> torch.Tensor:
    """x bf16 [B, Hi, Wi, C] -> the patch matrix [B*Ho*Wo, 9*C] of Conv2d(kernel 3, stride 2, padding 1), column order (dy, dx, c), at odd
    and even sizes (fluxmi_im2col3x3_s2)."""
    _req(x, torch.bfloat16, "x")
    x = x.contiguous()
    B, Hi, Wi, Cc = x.shape
    Ho, Wo = conv3x3_s2_hw(Hi, Wi)
    col = torch.empty((B * Ho * Wo, 9 * Cc), dtype=torch.bfloat16, device=x.device)
    call("fluxmi_im2col3x3_s2", _p(x), _p(col), B, Hi, Wi, Cc, _stream())
    return col


def conv3x3_s2(x: torch.Tensor, w2: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Conv2d(kernel 3, stride 2, padding 1) on NHWC bf16: x [B, Hi, Wi, C], w2 [Cout, 9*C] with K ordered (dy, dx, c) -> [B, Ho, Wo, Cout]:
    the symmetric-pad stride-2 patch matrix, then the bf16 GEMM."""
    B, Hi, Wi, _ = x.shape
    Ho, Wo = conv3x3_s2_hw(Hi, Wi)
    return linear(im2col3x3_s2(x), w2, bias).view(B, Ho, Wo, w2.shape[0])


def depth_head(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x bf16 [B, H, W, C] (a channel window is fine), w bf16 [C], bias bf16 [1] -> fp32 [B, H, W] = relu(x . w + bias), accumulated and
    stored in fp32 (fluxmi_depth_head: the head's last 1x1 convolution + ReLU)."""
    ldx = _depth_pixels(x, "depth_head", "x")
    _req(w, torch.bfloat16, "w")
    B, H, W, Cc = x.shape
    if w.numel() != Cc or not w.is_contiguous() or Cc % 8:
        raise ValueError(f"depth_head: w needs C = {Cc} contiguous entries, C a multiple of 8")
    out = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
    call("fluxmi_depth_head", _p(x), ldx, Cc, _p(w), _p(bias), _p(out), B * H * W, _stream())
    return out


def depth_to_map(depth: torch.Tensor, size, normalize: str = "minmax", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """depth fp32 [B, h, w] -> uint8 [B, H, W, 3], size = (H, W): half-pixel bilinear resize, normalisation, floor(v + 0.5) clamped to
    0..255, written to all three channels (fluxmi_depth_to_map).  normalize "minmax": each image's own min..max of the SOURCE depth -> 0..255
    (a constant image gives 0), from a deterministic two-launch reduction; "raw": clamp(depth, 0, 255).  `out`: a uint8 [B, H, W, 3] view
    with adjacent pixels (a window of a larger buffer is fine)."""
    _req(depth, torch.float32, "depth")
    if normalize not in DEPTH_NORMALIZE:
        raise ValueError(f"depth_to_map: normalize={normalize!r}: expected one of {tuple(DEPTH_NORMALIZE)}")
    if depth.ndim != 3 or min(depth.shape) < 1 or (depth.shape[2] > 1 and depth.stride(2) != 1):
        raise ValueError(f"depth_to_map: depth must be fp32 [B, h, w] with unit column stride, got {tuple(depth.shape)} / {depth.stride()}")
    B, h, w = depth.shape
    H, W = int(size[0]), int(size[1])
    if H < 1 or W < 1:
        raise ValueError(f"depth_to_map: size {tuple(size)} must be >= 1 x 1")
    ld = depth.stride(1) if h > 1 else w
    bs = depth.stride(0) if B > 1 else h * ld
    if ld < w or bs < h * ld:
        raise ValueError(f"depth_to_map: depth rows / images overlap (strides {depth.stride()})")
    out, old, obs = _u8_out(out, (B, H, W, 3), depth, "depth_to_map", "out", 3)
    nbytes = B * ((h * w + 4095) // 4096 + 1) * 8  # FLUXMI_DEPTH_MAP_WORK_BYTES
    work = torch.empty(nbytes // 4, dtype=torch.float32, device=depth.device)
    call("fluxmi_depth_to_map", _p(depth), ld, bs, _p(out), old, obs, _p(work), nbytes, B, h, w, H, W, DEPTH_NORMALIZE[normalize], _stream())
    return out
