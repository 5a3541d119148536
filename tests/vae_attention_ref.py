"""Reference, working-precision model and per-element error gate for the streaming VAE attention (csrc/vae_attention.hip,
include/fluxmi.h fluxmi_vae_attention) -- tests/attention_ref.py restated for one head of width D = 64 / 512 with a v bias.

  ref64          softmax(q k^T / sqrt D) v + b and A = softmax(...) |v| + |b| in fp64
  model          the same on the CPU with the header's rounding points, walked key tile by key tile (KEY_TILE keys), and nothing else;
                 `mut` names one deliberate defect (MUTANTS) for the test that the gate has the power to see it
  gate           what assert_close needs from the inputs alone
  assert_close   every element within 1.25 * max(1, r_model) * u (|ref| + A), rel-L2 within 1.25 x the model's
  inputs         the seeded input families the CPU mutation test and the GPU tests share

The gate is derived from the fp64 reference and the model only; nothing in it is measured on the kernel.  u = 2^-8 is the bf16 unit
roundoff; u |ref| is the rounding of the output, u A the rounding of every p_j to bf16 in the worst case.  r_model is the model's own worst
err / bound on the inputs at hand.  The factor 1.25 (attention_ref.MARGIN) covers what separates the kernel from the model: the fp32
summation order of the MFMA and of the row sum, v_exp_f32 and the fp32 division, all far below u.

q is [B, R, D] (R query rows; R = P in a self-attention, fewer when only some rows are checked), k and v are [B, P, D], the bias [D].
"""
import math

import torch

from attention_ref import MARGIN, U_BF16, _rel_l2, _worst_ratio

KEY_TILE = 64  # keys per tile of the kernel (include/fluxmi.h FLUXMI_VAE_ATTN_KEY_TILE)
FAMILIES = ("randn", "neg", "pos", "probe_last", "qzero")
MUTANTS = ("scale", "drop_last", "pad_key", "no_rescale", "no_bias", "swap_v")
BIAS_FREE_TAIL = 16  # probe_last: the last 16 probe columns carry no bias (see inputs)


def scale_log2(D):
    """the kernel's c = fp32(log2 e / sqrt D)"""
    return torch.tensor(1.4426950408889634 / math.sqrt(D), dtype=torch.float32)


def ref64(q, k, v, bias):
    """(ref, A) in fp64, [B, R, D]"""
    D = q.shape[-1]
    p = torch.softmax((q.double() @ k.double().transpose(1, 2)) / math.sqrt(D), dim=-1)
    return p @ v.double() + bias.double(), p @ v.double().abs() + bias.double().abs()


def poison_row(D):
    """what helper_refs.poison writes into a padded row: +-1e4, every third entry negative, as bf16 holds it"""
    return torch.where(torch.arange(D) % 3 == 0, -1.0e4, 1.0e4).bfloat16().float()


def model(q, k, v, bias, mut=None):
    """The header's arithmetic without the kernel's schedule: fp32 scores times c, per key tile the exact running maximum, O and l
    rescaled by exp2(m_old - m_new), p = exp2(t - m) in fp32 summed into l in fp32 and rounded to bf16 once for P V (fp32 accumulation);
    out = bf16(O / l + b).  bf16 [B, R, D].

    mut: scale (c 2 % too large) | drop_last (key P - 1 missing) | pad_key (key P admitted, holding the pad's poison in k and v) |
    no_rescale (O and l keep their scale when the maximum grows) | no_bias | swap_v (V rows P - 1 and P - 9 exchanged: two k-slots of one
    MFMA step)."""
    assert mut is None or mut in MUTANTS
    B, R, D = q.shape
    P = k.shape[1]
    c = scale_log2(D) * (torch.tensor(1.02, dtype=torch.float32) if mut == "scale" else 1.0)
    out = torch.empty(B, R, D, dtype=torch.bfloat16)
    for b in range(B):
        kf, vf = k[b].float(), v[b].float()
        if mut == "drop_last":
            kf, vf = kf[: P - 1], vf[: P - 1]
        elif mut == "pad_key":
            kf, vf = torch.cat((kf, poison_row(D)[None]), 0), torch.cat((vf, poison_row(D)[None]), 0)
        elif mut == "swap_v":
            vf = vf.clone()
            vf[[P - 1, P - 9]] = vf[[P - 9, P - 1]]
        t = (q[b].float() @ kf.T) * c
        m = torch.full((R, 1), -float("inf"))
        l, o = torch.zeros(R, 1), torch.zeros(R, D)
        for t0 in range(0, kf.shape[0], KEY_TILE):
            tt = t[:, t0 : t0 + KEY_TILE]
            m_new = torch.maximum(m, tt.max(dim=-1, keepdim=True).values)
            if mut != "no_rescale":
                alpha = torch.exp2(m - m_new)  # first tile: exp2(-inf) = 0 on O = l = 0
                l, o = l * alpha, o * alpha
            p = torch.exp2(tt - m_new)
            l = l + p.sum(dim=-1, keepdim=True)
            o = o + p.bfloat16().float() @ vf[t0 : t0 + KEY_TILE]
            m = m_new
        y = o / l
        if mut != "no_bias":
            y = y + bias.float()
        out[b] = y.bfloat16()
    return out


def gate(q, k, v, bias):
    ref, A = ref64(q, k, v, bias)
    bound = U_BF16 * (ref.abs() + A)
    mod = model(q, k, v, bias)
    return dict(ref=ref, A=A, bound=bound, r_model=_worst_ratio(mod, ref, bound), l2_model=_rel_l2(mod, ref))


def assert_close(got, g, what):
    """got: [B, R, D] holding bf16-rounded values; g: gate(q, k, v, bias).  Prints and returns the figures it compared."""
    got = got.detach().cpu()
    ref, bound = g["ref"], g["bound"]
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got.float()).all(), f"{what}: output not finite"
    r_got, l2_got = _worst_ratio(got, ref, bound), _rel_l2(got, ref)
    lim = MARGIN * max(1.0, g["r_model"])
    print(f"VAE_ATTN_BOUND {what}: model err/bound {g['r_model']:.3f} rel-L2 {g['l2_model']:.3e} | got err/bound {r_got:.3f} rel-L2 {l2_got:.3e}")
    n_bad = int(((got.double() - ref).abs() > lim * bound).sum())
    assert n_bad == 0, f"{what}: {n_bad} elements beyond {lim:.3f} x u (|ref| + A); worst err/bound {r_got:.3f} (model {g['r_model']:.3f})"
    assert l2_got <= MARGIN * g["l2_model"], f"{what}: rel-L2 {l2_got:.3e} > 1.25 x the model's {g['l2_model']:.3e}"
    return dict(r_model=g["r_model"], l2_model=g["l2_model"], r_got=r_got, l2_got=l2_got)


def inputs(family, B, P, D, seed):
    """Seeded bf16 q, k, v [B, P, D] and bias [D].
      randn        unit normal q, k, v, bias
      neg / pos    a common vector w, |w| = 1.5 sqrt D, added to every q and subtracted from / added to every k: every real score is about
                   -/+ 2.25 sqrt D, so a padded key at score 0 would take the whole softmax / the first tile's maximum jumps far up
      probe_last   unit-rms q, k rows; V one-hot on the last n = min(D, P) keys: output column c of a row is the softmax weight of key
                   P - n + c, so every key's weight and its k-slot in the V^T layout is checked by itself.  A bias of the weights' size or
                   more would widen the bound u (|ref| + A) past them, so it sits only on odd columns below n - 16 (and on the columns
                   >= n that probe nothing): the even columns and the last 16 probes are bias-free, the others show a missing bias
      qzero        q = 0: uniform weights 1 / P"""
    assert family in FAMILIES
    g = torch.Generator().manual_seed(seed * 1000003 + FAMILIES.index(family) * 7919 + P * 13 + D)
    rn = lambda *s: torch.randn(*s, generator=g)
    q, k, v, bias = rn(B, P, D), rn(B, P, D), rn(B, P, D), rn(D)
    if family in ("neg", "pos"):
        w = rn(D)
        w = w * (1.5 * math.sqrt(D) / w.norm())
        q = q + w
        k = k - w if family == "neg" else k + w
    elif family == "probe_last":
        q = q / q.pow(2).mean(-1, keepdim=True).sqrt()
        k = k / k.pow(2).mean(-1, keepdim=True).sqrt()
        n = min(D, P)
        v = torch.zeros(B, P, D)
        v[:, P - n + torch.arange(n), torch.arange(n)] = 1.0
        col = torch.arange(D)
        bias = torch.where(((col % 2 == 1) & (col < n - BIAS_FREE_TAIL)) | (col >= n), 0.5 * bias, torch.zeros(D))
    elif family == "qzero":
        q = torch.zeros_like(q)
    return q.bfloat16(), k.bfloat16(), v.bfloat16(), bias.bfloat16()
