"""The masked tile loop of the folded flow-attention kernel (csrc/attention2.hip, MASKED, fp16 K) restated on the CPU, schedule included,
and held to the per-element gate of tests/attention_mask_ref.py.  It checks the ARITHMETIC of the design where no GPU is needed:

  * the bias of a masked score (-32768 from the mask MFMA) added to an fp32 accumulator that starts from -M;
  * the running maximum M that starts from the floor (ops.ATTN_MASK_FLOOR, exp2 domain) instead of from tile 0's maximum;
  * the deferred rescale (a row moves to a new M only when its tile maximum exceeds M by more than 2^8; the branch is wave-uniform: when
    one of a wave's 32 rows triggers it, every row of the wave moves by max(its tile maximum - M, 0)), which multiplies the empty state
    of a row whose first tiles are all masked by exp2(-delta);
  * the tile skew: the bf16 fragments of P_{j-1} are still pending when the branch fires in step j and are re-rounded to bf16;
  * the documented operand range (include/fluxmi.h, ops.attention): rows whose admitted scores lie at the floor + 126 pass the gate; far
    below the floor - 126 a row sums to l = 0, which is why the range is documented.

The emulation is a model of the kernel, not the kernel: tests/test_attention_mask_gpu.py runs the same tables on the device."""
import math

import pytest
import torch

import attention_mask_ref as mr
import attention_ref as ar

KT = ar.KEY_TILE
FLOOR = -1024.0  # ops.ATTN_MASK_FLOOR, M_FLOOR of the kernel
DEFER = 8.0      # fluxmi_tuning_t.attn_defer_log2's default
WAVE_ROWS = 32   # query rows that share the wave-uniform rescale branch


def test_floor_constant_is_the_documented_one():
    from fluxmi import ops

    assert ops.ATTN_MASK_FLOOR == FLOOR and ops.ATTN_MASK_L_MAX == 12096
    # the staging of a masked launch (csrc/attention_common.h: 256 + 8192 + 128 (tiles + 1) bytes) behind 128 KiB of rings, within 160 KiB
    lds = lambda L: 131072 + 256 + 8192 + 128 * ((L + 63) // 64 + 1)
    assert lds(ops.ATTN_MASK_L_MAX) <= 160 * 1024 < lds(ops.ATTN_MASK_L_MAX + 1)


def emulate_masked_fold(q, k, v, allowed):
    """bf16 [B, L, H*128]: the folded masked kernel's step loop (deferred running max, the default build), one (b, h) at a time, all rows
    of a head at once"""
    B, H, L, D = q.shape
    out = torch.empty(B, H, L, D, dtype=torch.bfloat16)
    blocks = torch.arange(L) // WAVE_ROWS
    nblk = int(blocks.max()) + 1
    for b in range(B):
        bias = torch.where(allowed[b], torch.tensor(0.0), torch.tensor(-32768.0))
        for h in range(H):
            qs = (q[b, h].float() * ar.SCALE_LOG2).half().float()
            kf, vf = k[b, h].half().float(), v[b, h].float()
            tiles = [slice(t0, min(t0 + KT, L)) for t0 in range(0, L, KT)]
            score = lambda t, M: ((qs @ kf[t].T) - M) + bias[:, t]  # accumulator init -M, the QK^T chunks, then the mask MFMA
            s0 = score(tiles[0], torch.zeros(L, 1))
            M = torch.clamp(s0.max(dim=-1, keepdim=True).values, min=FLOOR)
            cur = s0 - M
            l, o, pend = torch.zeros(L, 1), torch.zeros(L, D), None
            for j, t in enumerate(tiles):
                mx = cur.max(dim=-1, keepdim=True).values
                fire = torch.zeros(nblk, dtype=torch.bool).index_put_((blocks,), (mx[:, 0] > DEFER), accumulate=True)[blocks][:, None]
                delta = torch.where(fire, mx.clamp(min=0.0), torch.zeros_like(mx))
                alpha = torch.exp2(-delta)
                l, o = l * alpha, o * alpha
                if pend is not None:
                    pend = torch.where(fire, (pend * alpha).bfloat16().float(), pend)
                cur, M = cur - delta, M + delta
                if pend is not None:
                    o = o + pend @ vf[tiles[j - 1]]
                nxt = score(tiles[j + 1], M) if j + 1 < len(tiles) else None  # S_{j+1} is produced with the M of this step
                p = torch.exp2(cur)
                l = l + p.sum(dim=-1, keepdim=True)
                pend, cur = p.bfloat16().float(), nxt
            o = o + pend @ vf[tiles[-1]]
            out[b, h] = (o / l).bfloat16()
    return ar.to_rows(out)


TABLES = dict(first=mr.table_first_tiles_masked, last=mr.table_last_tiles_masked, stripes=mr.table_stripes, regions=mr.table_two_regions)


@pytest.mark.parametrize("L", [100, 333, 448])
@pytest.mark.parametrize("which", sorted(TABLES))
def test_emulated_tile_loop_passes_the_gate(L, which):
    tab = TABLES[which](L)[None]
    allowed = mr.allowed_of(tab)
    for family in ("randn", "pos", "probe_last"):
        q, k, v = ar.attention_inputs(family, 1, 1, L, seed=41)
        gate = mr.masked_gate(q, k, v, allowed, True)
        ar.assert_attention_close(emulate_masked_fold(q, k, v, allowed), q, k, v, True, f"emulated L={L} {which} {family}", gate=gate)


def test_emulated_tile_loop_51_tiles_first_tiles_masked():
    L = 3264
    tab = mr.table_first_tiles_masked(L)[None]
    allowed = mr.allowed_of(tab)
    q, k, v = ar.attention_inputs("pos", 1, 1, L, seed=42)
    mr.assert_masked_close(emulate_masked_fold(q, k, v, allowed), q, k, v, allowed, True, "emulated L=3264 first tiles masked, pos")


def inputs_with_scores_near(level, L, seed):
    """q, k with every score q . k / sqrt(128) log2 e within a few units of `level` (exp2 domain): a common vector of opposite sign in q
    and k plus unit noise a tenth as large"""
    g = torch.Generator().manual_seed(seed)
    a = math.sqrt(abs(level) / float(ar.SCALE_LOG2) / 128)
    q = a + 0.1 * torch.randn(1, 1, L, 128, generator=g)
    k = -math.copysign(1.0, -level) * a + 0.1 * torch.randn(1, 1, L, 128, generator=g)
    v = torch.randn(1, 1, L, 128, generator=g)
    return q.bfloat16(), ar.flush_k(k.bfloat16()), v.bfloat16()


def test_documented_operand_range():
    """Every score at the documented lower end (floor + 126 in the exp2 domain): every row's M stays at the floor and the result passes the
    gate.  Every score below floor - 126 - 24 (exp2 of it is below the smallest fp32 denormal): l = 0 and the output is not finite -- the
    loss the header and ops.attention warn of."""
    L = 200
    tab = mr.table_first_tiles_masked(L)[None]
    allowed = mr.allowed_of(tab)
    q, k, v = inputs_with_scores_near(FLOOR + 126, L, seed=43)
    s = ((q[0, 0].float() * ar.SCALE_LOG2).half().float() @ k[0, 0].float().T)
    assert FLOOR + 100 < float(s.min()) and float(s.max()) < FLOOR + 152, (float(s.min()), float(s.max()))
    mr.assert_masked_close(emulate_masked_fold(q, k, v, allowed), q, k, v, allowed, True, "emulated, scores at the documented lower end")
    q, k, v = inputs_with_scores_near(FLOOR - 220, L, seed=43)
    assert not torch.isfinite(emulate_masked_fold(q, k, v, allowed)).all()
