"""What the native pre-LN transformer towers share -- SigLIP and CLIP vision (modules/image_embedders.py), DINOv2 (modules/depth.py) and the
CLIP text model (modules/conditioner.py): the weight cache, the load-time padding, one encoder layer, the patch embedding, the CLIP-style
`encoder.layers` skeleton and the image normaliser.  Plain functions; each tower keeps its own config handling, embeddings and layer loop.

One layer, as every tower launches it:  x += gate1 * out(attn(LN1(x)));  x += gate2 * fc2(act(fc1(LN2(x)))), each residual sum in the GEMM's
gate * y + x epilogue (the gate is ones, or DINOv2's LayerScale), q | k as one GEMM, V^T from the v-projection GEMM with its operands swapped,
the v bias added after P V (rows of P sum to 1).  T5 (RMS norm, no biases, a gated FF, a relative bias) is not one of these.
"""
from __future__ import annotations

from collections import namedtuple
from operator import attrgetter

import numpy as np
import torch
from torch import Tensor, nn


class _Weight(nn.Module):
    """A module that only owns `weight` (T5LayerNorm / relative_attention_bias / embeddings keep the HF key names)."""

    def __init__(self, *shape):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(*shape), requires_grad=False)


def _lin(i, o, bias):
    m = nn.Linear(i, o, bias=bias)
    m.requires_grad_(False)
    return m


class _Cache:
    """Fused / derived weights (a value of any type), rebuilt when a source parameter object or the sources' device changes."""

    def __init__(self):
        self._d = {}

    def get(self, key, srcs, fn):
        ent = self._d.get(key)
        if ent is None or len(ent[0]) != len(srcs) or any(a is not b for a, b in zip(ent[0], srcs)) or ent[1] != srcs[0].device:
            ent = (tuple(srcs), srcs[0].device, fn())
            self._d[key] = ent
        return ent[2]


def _bf(t: Tensor) -> Tensor:
    return t.detach().to(torch.bfloat16).contiguous()


def _round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def padded_head_dim(head_dim: int) -> int:
    """the head width fluxmi_vision_attention runs a head of `head_dim` at (64 or 96; SigLIP-so400m's 72 -> 96)"""
    if head_dim <= 64:
        return 64
    if head_dim <= 96:
        return 96
    raise ValueError(f"fluxmi: vision attention covers head_dim <= 96, got {head_dim}")


def pad_heads(t: Tensor, heads: int, hd: int, hp: int, dim: int = 0) -> Tensor:
    """rows (dim 0) or columns (dim 1) of H heads of hd -> H heads of hp, zero-filled per head (t itself when hp == hd)"""
    if hp == hd:
        return t
    if dim == 0:
        x = t.reshape(heads, hd, *t.shape[1:])
        out = x.new_zeros((heads, hp) + tuple(x.shape[2:]))
        out[:, :hd] = x
        return out.reshape(heads * hp, *t.shape[1:])
    x = t.reshape(t.shape[0], heads, hd)
    out = x.new_zeros(t.shape[0], heads, hp)
    out[:, :, :hd] = x
    return out.reshape(t.shape[0], heads * hp)


def unpad_heads(t: Tensor, heads: int, hd: int, hp: int, dim: int = 0) -> Tensor:
    if dim == 0:
        return t.reshape(heads, hp, *t.shape[1:])[:, :hd].reshape(heads * hd, *t.shape[1:])
    return t.reshape(t.shape[0], heads, hp)[:, :, :hd].reshape(t.shape[0], heads * hd)


def _pad_to(t: Tensor, n: int, dim: int = 0) -> Tensor:
    if t.shape[dim] == n:
        return t
    shape = list(t.shape)
    shape[dim] = n
    out = t.new_zeros(shape)
    out.narrow(dim, 0, t.shape[dim]).copy_(t)
    return out


def _linear_groups(rows_a, w, out_rows, bias=None, resid_rows=None, ones=None):
    """One GEMM launch over groups (<= 16 per launch): out_rows[i] = rows_a[i] . w^T (+ bias) (+ resid_rows[i], through the gate*y+x
    epilogue with a ones gate).  Each item is a 2-D view with unit column stride."""
    from fluxmi import _lib, ops

    N, K = w.shape
    epi = _lib.EPI_BF16 if resid_rows is None else _lib.EPI_GATE_RESID
    for i0 in range(0, len(rows_a), 16):
        gs = []
        for i in range(i0, min(i0 + 16, len(rows_a))):
            a, c = rows_a[i], out_rows[i]
            r = None if resid_rows is None else resid_rows[i]
            gs.append(ops.make_group(ops._p(a), ops._p(w), ops._p(bias), None, None, ops._p(c), a.shape[0], a.stride(0), c.stride(0),
                                     gate=ops._p(ones), resid=ops._p(r), ldr=r.stride(0) if r is not None else 0))
        ops.gemm_grouped(gs, N, K, False, _lib.E5M2, epi)


# ---- one layer's weights ----------------------------------------------------------------------------------------------------------------
# where a HF family keeps a layer's parts: the q / k / v / out projections, the two LayerNorms, fc1 / fc2 (modules) and, for DINOv2, the two
# LayerScale vectors (parameters)
LayerNames = namedtuple("LayerNames", "q k v out norm1 norm2 fc1 fc2 scale1 scale2", defaults=(None, None))
CLIP_LAYER = LayerNames("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "layer_norm1", "layer_norm2",
                        "mlp.fc1", "mlp.fc2")  # SigLIP, CLIP vision, CLIP text
DINOV2_LAYER = LayerNames("attention.attention.query", "attention.attention.key", "attention.attention.value", "attention.output.dense",
                          "norm1", "norm2", "mlp.fc1", "mlp.fc2", "layer_scale1.lambda1", "layer_scale2.lambda1")


def clip_encoder_layers(n: int, D: int, Fd: int, eps: float) -> nn.ModuleList:
    """`encoder.layers` of transformers' SigLIP / CLIP towers (the key names of CLIP_LAYER), n layers of width D with an MLP of Fd"""
    layers = nn.ModuleList()
    for _ in range(n):
        lay = nn.Module()
        lay.self_attn = nn.Module()
        for name in ("q_proj", "k_proj", "v_proj", "out_proj"):
            setattr(lay.self_attn, name, _lin(D, D, True))
        lay.layer_norm1, lay.layer_norm2 = nn.LayerNorm(D, eps=eps), nn.LayerNorm(D, eps=eps)
        lay.mlp = nn.Module()
        lay.mlp.fc1, lay.mlp.fc2 = _lin(D, Fd, True), _lin(Fd, D, True)
        layers.append(lay)
    return layers


def layer_weights(ck: _Cache, lay: nn.Module, spec: LayerNames, i, heads: int, hd: int, hp: int, mlp_pad: int) -> dict:
    """bf16 weights of layer `lay` (number i, of the family `spec`) as the kernels take them, built once through `ck`: heads of hd padded to
    hp (q | k fused; v's rows and bias; out's columns), fc1's rows / bias and fc2's columns padded to mlp_pad -- all pads zero, so exact.
    With hp == hd and mlp_pad == fc1's rows (the CLIP text model) they are the bf16 weights themselves."""
    q, k, v, o, n1, n2, fc1, fc2 = attrgetter(*spec[:8])(lay)
    ph = lambda t, dim=0: pad_heads(_bf(t), heads, hd, hp, dim).contiguous()  # noqa: E731
    p = dict(
        wqk=ck.get(("wqk", i), [q.weight, k.weight], lambda: torch.cat([ph(q.weight), ph(k.weight)], 0)),
        bqk=ck.get(("bqk", i), [q.bias, k.bias], lambda: torch.cat([ph(q.bias), ph(k.bias)], 0)),
        wv=ck.get(("wv", i), [v.weight], lambda: ph(v.weight)),
        bv=ck.get(("bv", i), [v.bias], lambda: ph(v.bias)),
        wo=ck.get(("wo", i), [o.weight], lambda: ph(o.weight, 1)),
        bo=ck.get(("bo", i), [o.bias], lambda: _bf(o.bias)),
        w1=ck.get(("w1", i), [fc1.weight], lambda: _pad_to(_bf(fc1.weight), mlp_pad, 0).contiguous()),
        b1=ck.get(("b1", i), [fc1.bias], lambda: _pad_to(_bf(fc1.bias), mlp_pad, 0).contiguous()),
        w2=ck.get(("w2", i), [fc2.weight], lambda: _pad_to(_bf(fc2.weight), mlp_pad, 1).contiguous()),
        b2=ck.get(("b2", i), [fc2.bias], lambda: _bf(fc2.bias)))
    vecs = [("g1", n1.weight), ("e1", n1.bias), ("g2", n2.weight), ("e2", n2.bias)]
    if spec.scale1 is not None:
        vecs += zip(("l1", "l2"), attrgetter(spec.scale1, spec.scale2)(lay))
    for name, t in vecs:
        p[name] = ck.get((name, i), [t], lambda t=t: _bf(t))
    return p


# ---- one layer's launches -----------------------------------------------------------------------------------------------------------------
def vision_attend(B: int, L: int, Lp: int, heads: int, hd: int, hp: int):
    """attend(h, qk, p) for B images of L tokens in Lp-row slabs: V^T = W_v . h_b^T per image (the weight is the GEMM's "A" operand, the
    image's rows its "W" operand; one launch per image), then fluxmi_vision_attention over all images, heads of hd run at width hp"""
    from fluxmi import ops

    def attend(h, qk, p):
        qk = qk.view(B, Lp, 2 * heads * hp)
        vt = torch.empty(B, heads * hp, Lp, dtype=torch.bfloat16, device=h.device)
        for b in range(B):
            ops.linear(p["wv"], h[b * Lp:(b + 1) * Lp], out=vt[b])
        o = ops.vision_attention(qk[:, :, : heads * hp], qk[:, :, heads * hp:], vt, L, heads, hp, hd ** -0.5, v_bias=p["bv"])
        return o.view(B * Lp, heads * hp)

    return attend


def text_attend(L: int, heads: int):
    """attend(h, qk, p) for one sequence of L tokens, heads of 64, causal (the CLIP text model): V^T, then fluxmi_text_attention"""
    from fluxmi import ops

    def attend(h, qk, p):
        vt = ops.linear(p["wv"], h)  # [H*64, Lp] = W_v . h^T, without its bias
        return ops.text_attention(qk[:, : heads * 64], qk[:, heads * 64:], vt, L, heads, scale=64 ** -0.5, causal=True, v_bias=p["bv"])

    return attend


def encoder_layer(x: Tensor, p: dict, attend, act, eps: float, gate1: Tensor, gate2: Tensor) -> Tensor:
    """one pre-LN layer on the rows x [rows, D] with layer_weights' dict p (the module docstring); `attend`: vision_attend / text_attend,
    `act`: the MLP's activation on fc1's output, gate1 / gate2: the gates of the two residual sums"""
    from fluxmi import _lib, ops

    h = ops.row_norm(x, p["g1"], p["e1"], eps=eps, rms=False)
    o = attend(h, ops.linear(h, p["wqk"], p["bqk"]), p)
    x = ops.linear(o, p["wo"], p["bo"], epilogue=_lib.EPI_GATE_RESID, gate=gate1, resid=x, out=torch.empty_like(x))
    h = ops.row_norm(x, p["g2"], p["e2"], eps=eps, rms=False)
    f = act(ops.linear(h, p["w1"], p["b1"]))
    return ops.linear(f, p["w2"], p["b2"], epilogue=_lib.EPI_GATE_RESID, gate=gate2, resid=x, out=torch.empty_like(x))


# ---- embeddings -----------------------------------------------------------------------------------------------------------------------------
def patch_embed(pix: Tensor, patch: int, gh: int, gw: int, patch_k: int, w: Tensor, bias, pos_rows: Tensor, cls_row, Lp: int,
                ones: Tensor) -> Tensor:
    """A stride-`patch` "valid" Conv2d + the position embedding: pix bf16 [B, C, H, W] -> x bf16 [B * Lp, D].  Each image has a zeroed Lp-row
    slab (zero rows stay finite through every layer): the class row `cls_row` first if there is one, then the gh gw patch rows
    bf16(pos_rows + bf16(conv)) -- the patch rows (fluxmi_patchify_rect, K padded to patch_k as w [D, patch_k] is) through one grouped GEMM
    with the position rows as its residual."""
    from fluxmi import ops

    B, G, r0 = pix.shape[0], gh * gw, 0 if cls_row is None else 1
    patches = ops.patchify_rect(pix, patch, gh, gw, patch_k)
    x = torch.zeros(B, Lp, w.shape[0], dtype=torch.bfloat16, device=pix.device)
    _linear_groups([patches[b * G:(b + 1) * G] for b in range(B)], w, [x[b, r0:r0 + G] for b in range(B)], bias,
                   resid_rows=[pos_rows] * B, ones=ones)
    if cls_row is not None:
        x[:, 0] = cls_row
    return x.view(B * Lp, -1)


def normalize_image(a, mean, std) -> Tensor:
    """a uint8 [H, W, 3] array -> fp32 [1, 3, H, W] on the host as transformers' image processors rescale and normalise: x * (1 / 255) in
    float64, then float32, then (x - mean) / std in float32 (mean, std: a float or one per channel)"""
    a = (np.asarray(a).astype(np.float64) * (1 / 255)).astype(np.float32)
    a = (a - np.asarray(mean, dtype=np.float32)) / np.asarray(std, dtype=np.float32)
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))[None]
