"""Reference and per-element error gate for the IP-Adapter term (csrc/ip_attention.hip), and the composed oracle of a forward with an adapter.

  qn_of            the block's image query after QK-RMSNorm, before RoPE: fo.rms_norm on the raw q (one bf16 rounding, as the kernel's helper)
  term_ref64       o = softmax(qn k_ip^T / sqrt(128)) v_ip in fp64 from the bf16 qn, with A = softmax(.) |v_ip| and E (below)
  assert_term_close   |o - ref| <= MARGIN * u * (|ref| + (1 + 2E) * A) for every element; MARGIN and u are tests/attention_ref.py's
  forward / denoise   fo.FluxOracle.forward with the term added behind every double block (XLabs' IPDoubleStreamBlockProcessor restated from
                      the oracle's own blocks: neither XLabs' code nor diffusers is available offline, so parity with them is unpinned)

The gate is derived from the fp64 reference alone.  u |ref| is the rounding of the output; u A would cover a bf16 rounding of every weight p_j
(the kernel keeps them in fp32, so this is slack).  The E term: the kernel's 1 / rms may differ from torch's rsqrt in the last fp32 bit, which
can move an element of qn by one bf16 ulp; every logit then moves by at most u * sum_d |qn_d k_jd| / sqrt(128) <= u E, a weight by a factor
exp(+-2 u E) relative to the others, the output by at most 2 u E A to first order.  E = max_j sum_d |qn_d k_jd| / sqrt(128) per (row, head).
"""
import math

import torch

import flux_oracle as fo
from attention_ref import MARGIN, U_BF16

HEAD = 128


def qn_of(q_raw, qn_scale):
    """q_raw bf16 [..., 128] -> bf16: fp32 rms_norm, eps 1e-6, times the learnable scale, one rounding (flux_oracle.rms_norm)"""
    return fo.rms_norm(q_raw, qn_scale)


def term_ref64(q_raw, qn_scale, k_ip, v_ip, nk=None, scale_logits=True, use_norm_scale=True):
    """q_raw bf16 [B, rows, heads*128]; k_ip, v_ip bf16 [B, >= nk, heads*128] -> (ref, A, E) fp64 [B, rows, heads*128] (E broadcast over a head's
    128 columns).  scale_logits / use_norm_scale = False build the wrong terms the CPU mutation test feeds to the gate."""
    B, R, HD = q_raw.shape
    H = HD // HEAD
    nk = k_ip.shape[1] if nk is None else nk
    w = qn_scale if use_norm_scale else torch.ones_like(qn_scale)
    qn = qn_of(q_raw.reshape(B, R, H, HEAD), w).double().permute(0, 2, 1, 3)            # [B, H, R, 128]
    k = k_ip[:, :nk].reshape(B, nk, H, HEAD).double().permute(0, 2, 1, 3)                # [B, H, nk, 128]
    v = v_ip[:, :nk].reshape(B, nk, H, HEAD).double().permute(0, 2, 1, 3)
    c = 1.0 / math.sqrt(HEAD) if scale_logits else 1.0
    p = torch.softmax((qn @ k.transpose(-1, -2)) * c, dim=-1)
    ref = p @ v
    A = p @ v.abs()
    E = (qn.abs() @ k.abs().transpose(-1, -2)).max(dim=-1, keepdim=True).values / math.sqrt(HEAD)  # [B, H, R, 1]
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(B, R, HD)
    return rows(ref), rows(A), rows(E.expand(-1, -1, -1, HEAD))


def term_bound(ref, A, E):
    return MARGIN * U_BF16 * (ref.abs() + (1.0 + 2.0 * E) * A)


def gate_violations(got, ref, A, E):
    """number of elements beyond the gate, and the worst err / bound (an element whose bound is 0 must be exact)"""
    err = (got.detach().cpu().double() - ref).abs()
    bound = term_bound(ref, A, E)
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return int((err > bound).sum()), float(r.max())


def assert_term_close(got, ref, A, E, what):
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got.float()).all(), f"{what}: output not finite"
    n_bad, worst = gate_violations(got, ref, A, E)
    print(f"IP_BOUND {what}: worst err / bound {worst:.3f} (bound = {MARGIN} u (|ref| + (1 + 2E) A))")
    assert n_bad == 0, f"{what}: {n_bad} elements beyond the gate; worst err / bound {worst:.3f}"


def term_sdpa_bf16(q_raw, qn_scale, k_ip, v_ip, nk=None):
    """torch's CPU bf16 SDPA on the bf16 qn: what a PyTorch implementation of the adapter computes (the reference the gate must admit)"""
    B, R, HD = q_raw.shape
    H = HD // HEAD
    nk = k_ip.shape[1] if nk is None else nk
    qn = qn_of(q_raw.reshape(B, R, H, HEAD), qn_scale).permute(0, 2, 1, 3)
    k = k_ip[:, :nk].reshape(B, nk, H, HEAD).permute(0, 2, 1, 3)
    v = v_ip[:, :nk].reshape(B, nk, H, HEAD).permute(0, 2, 1, 3)
    o = torch.nn.functional.scaled_dot_product_attention(qn, k, v)
    return o.permute(0, 2, 1, 3).reshape(B, R, HD)


# the kernel cases shared by the CPU gate test and the GPU tests: (rows, heads, nk, B), the whole grid.  rows: one lane pair, a ragged wave,
# half a workgroup, two workgroups + 1; heads 1 / 3 / 24 (Flux-dev); Nk 1 (a softmax of one), 4 (XLabs v1), 5 (odd), 16, 64 (the LDS limit)
KERNEL_CASES = [(rows, heads, nk, B) for rows in (1, 5, 64, 257) for heads in (1, 3, 24) for nk in (1, 4, 5, 16, 64) for B in (1, 3)]


def term_inputs(rows, heads, nk, B, seed, nk_alloc=None):
    """seeded bf16 raw q [B, rows, heads*128] (rms ~ 3: the norm matters), qn scale [128] around 1, k_ip / v_ip [B, nk_alloc, heads*128]"""
    g = torch.Generator().manual_seed(seed * 7919 + rows * 131 + heads * 17 + nk)
    nk_alloc = nk if nk_alloc is None else nk_alloc
    q = (3.0 * torch.randn(B, rows, heads * HEAD, generator=g)).bfloat16()
    w = (1.0 + 0.25 * torch.randn(HEAD, generator=g)).bfloat16()
    k = torch.randn(B, nk_alloc, heads * HEAD, generator=g).bfloat16()
    v = torch.randn(B, nk_alloc, heads * HEAD, generator=g).bfloat16()
    return q, w, k, v


# ---- composed oracle ------------------------------------------------------------------------------------------------------------------
def block_term(oracle, i, trace, k_ip, v_ip):
    """the adapter term of double block i from the block's traced img_qkv: bf16 [B, Li, H]; k_ip, v_ip bf16 [B, nk, H]"""
    pre = f"double_blocks.{i}"
    H = oracle.p.num_heads
    iq = fo.split_heads(trace[pre + ".img_qkv"], H)[0]                                   # [B, heads, Li, 128]
    qn = fo.rms_norm(iq, oracle.sd[pre + ".img_attn.norm.query_norm.scale"])
    B, nk = k_ip.shape[0], k_ip.shape[1]
    k = k_ip.reshape(B, nk, H, HEAD).permute(0, 2, 1, 3)
    v = v_ip.reshape(B, nk, H, HEAD).permute(0, 2, 1, 3)
    o = fo.attention_fp64(qn, k, v).to(qn.dtype).transpose(1, 2)                          # softmax in fp64, one rounding
    return o.reshape(*o.shape[:-2], -1)


def forward(main, img, img_ids, txt, txt_ids, timesteps, y, guidance, k_ip=None, v_ip=None, scales=None, cn=None):
    """main.forward with the adapter term behind every double block: img = img + o_i * s[b, i] on bf16 tensors, i.e. bf16(img + bf16(o * s)).
    k_ip, v_ip: bf16 [depth, B, nk, H]; scales: float [B, depth].  cn = (Rd, Rs, s): ControlNet residuals (controlnet_ref) added behind the
    term, in the engine's order block, adapter, ControlNet.  k_ip None: main.forward itself."""
    import controlnet_ref as cr

    h = main.lin["img_in"](img)
    vec = main.embed_vec(timesteps, y, guidance)
    t = main.lin["txt_in"](txt)
    pe = fo.rope_table(torch.cat((txt_ids, img_ids), 1), main.p.axes_dim, main.p.theta, main.dtype)
    for i in range(main.p.depth):
        trace = {} if k_ip is not None else None
        h, t = main.double_block(i, h, t, vec, pe, trace)
        if k_ip is not None:
            o = block_term(main, i, trace, k_ip[i], v_ip[i])
            s = torch.as_tensor(scales, dtype=torch.float32)[:, i]
            h = h + (o.float() * s[:, None, None]).to(o.dtype)
        if cn is not None and cn[0]:
            h = h + cn[0][cr.block_index(i, main.p.depth, len(cn[0]))] * float(cn[2])
    Lt = t.shape[1]
    x = torch.cat((t, h), 1)
    for i in range(main.p.depth_single_blocks):
        x = main.single_block(i, x, vec, pe)
        if cn is not None and cn[1]:
            x = torch.cat((x[:, :Lt], x[:, Lt:] + cn[1][cr.block_index(i, main.p.depth_single_blocks, len(cn[1]))] * float(cn[2])), 1)
    return main.final_layer(x[:, Lt:], vec)


def denoise(main, img, img_ids, txt, txt_ids, y, timesteps, guidance=3.5, k_ip=None, v_ip=None, scales=None):
    """fo.denoise over `forward`"""
    B = img.shape[0]
    g = torch.full((B,), guidance, dtype=main.dtype)
    for t_curr, t_prev in zip(timesteps[:-1], timesteps[1:]):
        t_vec = torch.full((B,), t_curr, dtype=main.dtype)
        img = img + (t_prev - t_curr) * forward(main, img, img_ids, txt, txt_ids, t_vec, y, g, k_ip, v_ip, scales)
    return img


def denoise_guided(main, img, img_ids, txt, txt_ids, y, neg_txt, neg_y, timesteps, guidance, cfg_scale, k_ip, v_ip, scales):
    """the guided loop (fluxmi_engine_denoise_cfg): both branches in one batch of 2B with their own K / V [depth, 2B, nk, H] and scales
    [2B, depth], prompt branches first; x += bf16(dt * (u + s (c - u))) with one bf16 rounding per operation"""
    B = img.shape[0]
    g = torch.full((2 * B,), guidance, dtype=main.dtype)
    tx, yy = torch.cat((txt, neg_txt), 0), torch.cat((y, neg_y), 0)
    ii, ti = torch.cat((img_ids, img_ids), 0), torch.cat((txt_ids, txt_ids), 0)
    for t_curr, t_prev in zip(timesteps[:-1], timesteps[1:]):
        t_vec = torch.full((2 * B,), t_curr, dtype=main.dtype)
        pred = forward(main, torch.cat((img, img), 0), ii, tx, ti, t_vec, yy, g, k_ip, v_ip, scales)
        c, u = pred[:B], pred[B:]
        img = img + (t_prev - t_curr) * (u + cfg_scale * (c - u))
    return img
