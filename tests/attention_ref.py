"""Reference, working-precision model and per-element error gate for the flow attention (csrc/attention2.hip; flux_model.py:41-45).

  attention_ref64          softmax(q k^T / sqrt(128)) v and A = softmax(...) |v| in fp64
  attention_model          the same on the CPU with the kernel's DOCUMENTED rounding points and nothing else (exact=True: plus the second
                           bf16 rounding of a pending P tile in the exact-running-max build, see there)
  assert_attention_close   every element within 1.25 * max(1, r_model) * u (|ref| + A), rel-L2 within 1.25 x the model's
  attention_inputs         the seeded input families the CPU mutation test and the GPU edge tests share

The gate is derived from the fp64 reference and the model only; nothing in it is measured on the kernel.  u = 2^-8 is the bf16 unit
roundoff; u |ref| is the rounding of the output, u A the rounding of every p_j to bf16 in the worst case (all errors aligned with the
signs of v).  r_model is the model's own worst err / bound on the inputs at hand: it is 1 up to second-order terms unless the fp16
rounding of the folded Q matters (rows that score ~100 against a spiked key).  The factor 1.25 covers what separates the kernel from the
model: fp32 summation order and v_exp_f32, both far below u, and the deferred running max -- P on a grid up to 2^8 higher with the same
relative rounding, but a row's largest weight is then no longer exactly 1 and carries a rounding error of its own: on peaky rows the
default build's rel-L2 was measured at up to 1.22 x the model's (profiles/attention_bound.txt), inside the factor.  All tensors are [B, H, L, 128] on the way in and [B, L, H*128] (the kernels' output layout) on the way out.
"""
import math

import torch

U_BF16 = 2.0 ** -8
MARGIN = 1.25
KEY_TILE = 64  # keys per tile of the kernel (csrc/attention_common.h KT)
SCALE_LOG2 = torch.tensor(0.08838834764831845, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)  # csrc/attention.hip
FAMILIES = ("randn", "neg", "pos", "probe_last", "probe_first", "qzero")  # probe_first: L > 128 only


def to_rows(x):
    """[B, H, L, 128] -> [B, L, H*128]"""
    B, H, L, D = x.shape
    return x.transpose(1, 2).reshape(B, L, H * D)


def flush_k(k):
    """below fp16's normal range a bf16 value is not exact in fp16 (the engine's K is RMS-normalised: |k| ~ 1)"""
    return torch.where(k.abs() < 6.2e-5, torch.zeros_like(k), k)


def attention_ref64(q, k, v):
    """(ref, A) in fp64, head by head (an fp64 score matrix of L = 4608 is 170 MB)."""
    B, H, L, D = q.shape
    ref = torch.empty(B, H, L, D, dtype=torch.float64)
    A = torch.empty(B, H, L, D, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            p = torch.softmax((q[b, h].double() @ k[b, h].double().T) / math.sqrt(D), dim=-1)
            ref[b, h] = p @ v[b, h].double()
            A[b, h] = p @ v[b, h].double().abs()
    return to_rows(ref), to_rows(A)


def attention_model(q, k, v, fold, exact=False):
    """The kernel's arithmetic without its schedule: fp32 scores (fold: Q * 128^-0.5 log2 e rounded to fp16 first, attention_common.h
    load_q_frags), exact row max, P = exp2(s - m) in fp32, row sum from the fp32 P, P rounded to bf16 for P V, fp32 accumulation, one bf16
    rounding of O / l.  bf16 [B, L, H*128].

    exact: the build with exact running-max tracking (fluxmi_tuning_t.attn_var bit 1) has one more rounding point.  The kernel is skewed
    by one 64-key tile -- the bf16 fragments of P_{j-1} are still pending when the row max of tile j is known -- and when a row's max
    grows there, the rescale branch multiplies O, l AND those pending bf16 fragments by alpha = exp2(m_old - m_new) and rounds them to
    bf16 a second time (csrc/attention2.hip, rescale_state: `pp[i][e] = pack_bf2(... * alpha, ... * alpha)`).  With exact tracking that
    happens in most early tiles of a row; with the deferred max (the default) only when a row max grows by more than 2^8, where the
    re-rounded weights are below 2^-8 of the row's largest.  exact=True walks the key tiles and applies that second rounding."""
    B, H, L, D = q.shape
    out = torch.empty(B, H, L, D, dtype=torch.bfloat16)
    c = SCALE_LOG2
    for b in range(B):
        for h in range(H):
            kf, vf = k[b, h].float(), v[b, h].float()
            if fold:
                s = (q[b, h].float() * c).half().float() @ kf.T
            else:
                s = (q[b, h].float() @ kf.T) * c
            if not exact:
                p = torch.exp2(s - s.max(dim=-1, keepdim=True).values)
                l = p.sum(dim=-1, keepdim=True)
                o = p.bfloat16().float() @ vf
            else:
                m = torch.full((L, 1), -float("inf"))
                l, o, pend = torch.zeros(L, 1), torch.zeros(L, D), None
                for t0 in range(0, L, KEY_TILE):
                    st = s[:, t0 : t0 + KEY_TILE]
                    m_new = torch.maximum(m, st.max(dim=-1, keepdim=True).values)
                    alpha = torch.exp2(m - m_new)  # 1 for a row whose max did not grow: its pending fragments keep their bits
                    l, o = l * alpha, o * alpha
                    if pend is not None:
                        o = o + (pend * alpha).bfloat16().float() @ vf[t0 - KEY_TILE : t0]
                    p = torch.exp2(st - m_new)
                    l = l + p.sum(dim=-1, keepdim=True)
                    pend, m = p.bfloat16().float(), m_new
                o = o + pend @ vf[(L - 1) // KEY_TILE * KEY_TILE :]
            out[b, h] = (o / l).bfloat16()
    return to_rows(out)


def _rel_l2(x, ref):
    n = ref.norm().item()
    return ((x.double() - ref).norm().item() / n) if n > 0 else float((x.double() - ref).norm().item() > 0)


def _worst_ratio(x, ref, bound):
    """max err / bound; an element whose bound is 0 (every V it can see is 0) must be exact"""
    err = (x.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)  # x / 0 = inf for x > 0
    return r.max().item()


def attention_gate(q, k, v, fold, exact=False, ref_A=None):
    """what assert_attention_close needs from the inputs alone: compute once, check several kernel builds against it"""
    ref, A = attention_ref64(q, k, v) if ref_A is None else ref_A
    bound = U_BF16 * (ref.abs() + A)
    model = attention_model(q, k, v, fold, exact)
    return dict(ref=ref, A=A, bound=bound, r_model=_worst_ratio(model, ref, bound), l2_model=_rel_l2(model, ref))


def assert_attention_close(got, q, k, v, fold, what, gate=None, exact=False):
    """got: [B, L, H*128] (bf16 kernel output, or any tensor holding bf16-rounded values); exact: got comes from the exact-running-max
    build (attention_model).  gate: attention_gate(q, k, v, fold, exact) if already computed.  Returns the figures it compared."""
    g = attention_gate(q, k, v, fold, exact) if gate is None else gate
    got = got.detach().cpu()
    ref, bound = g["ref"], g["bound"]
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{what}: output not finite"
    r_got, l2_got = _worst_ratio(got, ref, bound), _rel_l2(got, ref)
    lim = MARGIN * max(1.0, g["r_model"])
    stats = dict(r_model=g["r_model"], l2_model=g["l2_model"], r_got=r_got, l2_got=l2_got)
    print(f"ATTN_BOUND {what}: model err/bound {g['r_model']:.3f} rel-L2 {g['l2_model']:.3e} | got err/bound {r_got:.3f} rel-L2 {l2_got:.3e}")
    n_bad = int(((got.double() - ref).abs() > lim * bound).sum())
    assert n_bad == 0, f"{what}: {n_bad} elements beyond {lim:.3f} x u (|ref| + A); worst err/bound {r_got:.3f} (model {g['r_model']:.3f})"
    assert l2_got <= MARGIN * g["l2_model"], f"{what}: rel-L2 {l2_got:.3e} > 1.25 x the model's {g['l2_model']:.3e}"
    return stats


def attention_inputs(family, B, H, L, seed):
    """Seeded bf16 q, k, v [B, H, L, 128]; |k| below fp16's normal range flushed, so bf16 K and fp16 K hold the same values.
      randn        unit normal q, k, v
      neg / pos    a common vector w, |w| = 1.5 sqrt(128), added to every q and subtracted from / added to every k: every real score is
                   about -25 / +25, so a padded key at score 0 would take the whole softmax / the first tile's maximum jumps far above 2^8
      probe_last   unit-rms q, k rows; V one-hot on the last min(128, L) keys: output column c of a row is the softmax weight of key
      probe_first  L - min(128, L) + c (probe_first: of key c), so every key's weight and its k-slot in the V^T layout is checked by itself
      qzero        q = 0: uniform weights 1 / L"""
    assert family in FAMILIES
    g = torch.Generator().manual_seed(seed * 1000003 + FAMILIES.index(family) * 7919 + L)
    rn = lambda: torch.randn(B, H, L, 128, generator=g)
    q, k, v = rn(), rn(), rn()
    if family in ("neg", "pos"):
        w = torch.randn(128, generator=g)
        w = w * (1.5 * math.sqrt(128) / w.norm())
        q = q + w
        k = k - w if family == "neg" else k + w
    elif family in ("probe_last", "probe_first"):
        q = q / q.pow(2).mean(-1, keepdim=True).sqrt()
        k = k / k.pow(2).mean(-1, keepdim=True).sqrt()
        n = min(128, L)
        k0 = L - n if family == "probe_last" else 0
        v = torch.zeros(B, H, L, 128)
        v[:, :, k0 + torch.arange(n), torch.arange(n)] = 1.0
    elif family == "qzero":
        q = torch.zeros_like(q)
    return q.bfloat16(), flush_k(k.bfloat16()), v.bfloat16()


def families_for(L):
    return [f for f in FAMILIES if f != "probe_first" or L > 128]
