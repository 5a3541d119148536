"""Masked counterparts of tests/attention_ref.py for the token-group masks of fluxmi_attention_grouped (csrc/attention2.hip, MASKED).

  allowed_of               descriptors [B, L] -> bool [B, L, L]: query i attends key j iff bit g_j of P_i (include/fluxmi.h)
  attention_ref64_masked   softmax over the allowed keys only, in fp64: (ref, A) like attention_ref64
  attention_model_masked   attention_model's rounding points (fold: fp16 Q * scale; fp32 scores; exact row max over the ALLOWED keys; P in fp32
                           for the row sum, bf16 for P V; one bf16 rounding of O / l) with the disallowed keys removed -- the mask adds no
                           rounding point: an admitted score receives +0 in the accumulator, a masked one has P = 0 exactly
  masked_gate              attention_gate with those two; feed it to attention_ref.assert_attention_close(gate=...), whose arithmetic
                           (1.25 max(1, r_model) u (|ref| + A), rel-L2 <= 1.25 x the model's) is used unchanged.  A column none of whose
                           allowed keys has a non-zero V has bound 0 and must be exactly 0.
  tables                   the descriptor tables the CPU mutation test and the GPU test share

Nothing here is measured on the kernel."""
import math

import torch

import attention_ref as ar

GROUPS = 16


def desc(group, perm):
    """int64 descriptors (g | P << 16) from key groups and permission bit sets"""
    return group.to(torch.int64) | (perm.to(torch.int64) << 16)


def to_i32(d):
    """the 32 descriptor bits as the int32 tensor the ops take"""
    d = d.to(torch.int64) & 0xFFFFFFFF
    return torch.where(d >= 1 << 31, d - (1 << 32), d).to(torch.int32)


def split_desc(d):
    d = d.to(torch.int64) & 0xFFFFFFFF
    return d & 15, d >> 16


def allowed_of(d):
    g, p = split_desc(d)
    return ((p[..., :, None] >> g[..., None, :]) & 1).bool()


def self_admitting(d):
    g, p = split_desc(d)
    return bool(((p >> g) & 1).all())


def attention_ref64_masked(q, k, v, allowed):
    B, H, L, D = q.shape
    ref = torch.empty(B, H, L, D, dtype=torch.float64)
    A = torch.empty(B, H, L, D, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            s = (q[b, h].double() @ k[b, h].double().T) / math.sqrt(D)
            p = torch.softmax(s.masked_fill(~allowed[b], -float("inf")), dim=-1)
            ref[b, h] = p @ v[b, h].double()
            A[b, h] = p @ v[b, h].double().abs()
    return ar.to_rows(ref), ar.to_rows(A)


def attention_model_masked(q, k, v, allowed, fold):
    B, H, L, D = q.shape
    out = torch.empty(B, H, L, D, dtype=torch.bfloat16)
    c = ar.SCALE_LOG2
    for b in range(B):
        for h in range(H):
            kf, vf = k[b, h].float(), v[b, h].float()
            if fold:
                s = (q[b, h].float() * c).half().float() @ kf.T
            else:
                s = (q[b, h].float() @ kf.T) * c
            s = s.masked_fill(~allowed[b], -float("inf"))
            p = torch.exp2(s - s.max(dim=-1, keepdim=True).values)
            l = p.sum(dim=-1, keepdim=True)
            out[b, h] = ((p.bfloat16().float() @ vf) / l).bfloat16()
    return ar.to_rows(out)


def masked_gate(q, k, v, allowed, fold, ref_A=None):
    ref, A = attention_ref64_masked(q, k, v, allowed) if ref_A is None else ref_A
    bound = ar.U_BF16 * (ref.abs() + A)
    model = attention_model_masked(q, k, v, allowed, fold)
    return dict(ref=ref, A=A, bound=bound, r_model=ar._worst_ratio(model, ref, bound), l2_model=ar._rel_l2(model, ref))


def assert_masked_close(got, q, k, v, allowed, fold, what, gate=None):
    g = masked_gate(q, k, v, allowed, fold) if gate is None else gate
    return ar.assert_attention_close(got, q, k, v, fold, what, gate=g)


# ---- tables -------------------------------------------------------------------------------------------------------------------------------
def table_all(L):
    """every query admits every group; keys spread over all 16 groups"""
    g = torch.arange(L) % GROUPS
    return desc(g, torch.full((L,), 0xFFFF))


def table_segments(L, edges, perms):
    """keys [edges[i-1], edges[i]) form group i; perms[i] = permission set of the queries of segment i"""
    g = torch.bucketize(torch.arange(L), torch.tensor(list(edges)), right=True)
    assert int(g.max()) < len(perms)
    return desc(g, torch.tensor(list(perms))[g])


def table_first_tiles_masked(L, n_tiles=2):
    """rows >= L/2 admit none of the first n_tiles key tiles: group 0 = those keys (when L leaves keys behind them), group 1 = the rest.
    Rows of group 0 see everything.  The masked rows run the first tiles with an empty softmax state."""
    cut = min(n_tiles * ar.KEY_TILE, L // 2)
    g = (torch.arange(L) >= cut).long()
    half = torch.arange(L) >= max(L // 2, cut)
    perm = torch.where(half, torch.tensor(0b10), torch.tensor(0b11))
    return desc(g, perm)


def table_last_tiles_masked(L, n_tiles=2):
    """rows < L/2 admit none of the keys from the tile of key L - n_tiles * 64 on"""
    cut = max(L - n_tiles * ar.KEY_TILE, L // 2)
    g = (torch.arange(L) >= cut).long()
    perm = torch.where(torch.arange(L) < min(L // 2, cut), torch.tensor(0b01), torch.tensor(0b11))
    return desc(g, perm)


def table_stripes(L):
    """the sparsest legal mask: key j in group j % 16, every query admits its own group only"""
    g = torch.arange(L) % GROUPS
    return desc(g, 1 << g)


def table_two_regions(L):
    """what the CPU mutants act on: base text | region-1 text | region-2 text | image tokens under {1}, {1, 2}, {2}, {} in bands, with
    the last 128 keys (the probe_last columns) cut by three segment edges.  Groups 0..2 text, 3..6 the four coverage patterns."""
    n_txt = min(48, L // 2)
    e = [n_txt // 3, 2 * n_txt // 3, n_txt]
    n_img = L - n_txt
    img_e = [n_txt + (n_img * i) // 4 for i in (1, 2, 3)]
    g = torch.bucketize(torch.arange(L), torch.tensor(e + img_e), right=True)
    IMG = 0b1111000
    perms = [0b0000001 | IMG,            # base text: itself + every image group
             0b0000010 | 0b0011000,      # region-1 text: itself + image groups whose pattern holds 1 (groups 3, 4)
             0b0000100 | 0b0110000,      # region-2 text: itself + groups 4, 5
             0b0000001 | 0b010 | IMG,    # image under {1}
             0b0000001 | 0b110 | IMG,    # image under {1, 2}
             0b0000001 | 0b100 | IMG,    # image under {2}
             0b0000001 | IMG]            # image under {}
    return desc(g, torch.tensor(perms)[g])
