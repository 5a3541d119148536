"""The attention gate of tests/attention_ref.py discriminates: the working-precision model passes it on every input family, and every
listed mutant of the fp64 reference (rounded to bf16 -- a kernel that is wrong in that one way and otherwise perfect) is rejected by at
least one family at every sequence length.  CPU only; this is the evidence that a kernel which passes test_attention_edges
(tests/test_ops_gpu.py) has the softmax scale, the ragged-tile mask, the k-slot permutation of V^T and the head indexing right."""
import math

import pytest
import torch

import attention_ref as ar
import flux_oracle as fo
from parity_util import round_fp64_to_bf16

LENGTHS = [2, 33, 64, 65, 129, 320, 1100, 4608]


def _softmax_pv(q, k, v, scale=1.0, extra_zero_keys=0, drop_last=False):
    """fp64 attention [B, L, H*128] with the mutations that act on the scores"""
    B, H, L, D = q.shape
    out = torch.empty(B, H, L, D, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            kk, vv = k[b, h].double(), v[b, h].double()
            if drop_last:
                kk, vv = kk[:-1], vv[:-1]
            if extra_zero_keys:
                kk = torch.cat((kk, torch.zeros(extra_zero_keys, D, dtype=torch.float64)))
                vv = torch.cat((vv, torch.zeros(extra_zero_keys, D, dtype=torch.float64)))
            out[b, h] = torch.softmax(scale * (q[b, h].double() @ kk.T) / math.sqrt(D), dim=-1) @ vv
    return ar.to_rows(out)


def _mutants(L, H):
    m = {
        "scale x 1.02": lambda q, k, v: _softmax_pv(q, k, v, scale=1.02),
        "last key dropped": lambda q, k, v: _softmax_pv(q, k, v, drop_last=True),
    }
    if L % 64:
        m["one zero key admitted"] = lambda q, k, v: _softmax_pv(q, k, v, extra_zero_keys=1)
        m["all padding keys admitted"] = lambda q, k, v: _softmax_pv(q, k, v, extra_zero_keys=(L + 63) // 64 * 64 - L)
    g0 = 16 * ((L - 2) // 16)
    a, b = g0, min(g0 + 4, L - 1)  # two keys of one 16-key group (bit 2 set / clear: the pair the V^T layout exchanges)

    def swapped(q, k, v):
        v2 = v.clone()
        v2[:, :, a], v2[:, :, b] = v[:, :, b], v[:, :, a]
        return _softmax_pv(q, k, v2)

    m["two V rows of a 16-key group exchanged"] = swapped
    if H == 2:
        m = {"heads exchanged": lambda q, k, v: _softmax_pv(q, k, v.flip(1))}
    return m


def _rejected(mut, q, k, v, fold, gate, what):
    try:
        ar.assert_attention_close(round_fp64_to_bf16(mut), q, k, v, fold, what, gate=gate)
    except AssertionError:
        return True
    return False


def test_ref64_extends_the_oracle():
    """attention_ref64's first output is fo.attention_fp64 in the kernels' output layout; A bounds it"""
    q, k, v = ar.attention_inputs("randn", 2, 3, 97, seed=5)
    ref, A = ar.attention_ref64(q, k, v)
    assert (ref - ar.to_rows(fo.attention_fp64(q, k, v))).abs().max().item() <= 1e-14
    assert (ref.abs() <= A).all()


@pytest.mark.parametrize("L", LENGTHS)
def test_model_passes_and_mutants_fail(L):
    torch.manual_seed(0)
    report = []
    for H in (1, 2):
        fams = ar.families_for(L) if H == 1 else ["randn"]  # the probe's V is the same in every head: only dense V tells heads apart
        mutants = _mutants(L, H)
        caught = {name: [] for name in mutants}
        for fam in fams:
            q, k, v = ar.attention_inputs(fam, 1, H, L, seed=11)
            assert torch.equal(k.half().float(), k.float())
            ref_A = ar.attention_ref64(q, k, v)
            gates = {(fold, exact): ar.attention_gate(q, k, v, fold, exact, ref_A=ref_A) for fold in (False, True) for exact in (False, True)}
            for (fold, exact), g in gates.items():
                # the model against its own gate.  Its distance from the bound u (|ref| + A) is what may widen the gate, so it is limited here:
                # the documented rounding points give 1 + second-order terms + the fp16 rounding of a folded Q; the second bf16 rounding of P
                # in the exact-max build (attention_model) puts 2 u A beside u |ref|, i.e. at most 1.5 where |ref| = A (the probes)
                ar.assert_attention_close(ar.attention_model(q, k, v, fold, exact), q, k, v, fold, f"model {fam} L={L} H={H} fold={fold} exact={exact}", gate=g)
                assert g["r_model"] <= (1.5 if exact else 1.1), f"{fam} L={L} fold={fold} exact={exact}: the model itself sits at {g['r_model']:.3f} x the bound"
            for name, fn in mutants.items():
                mut = fn(q, k, v)
                # a mutant counts as rejected by a family only if the gates of ALL four builds reject it (the GPU test runs all four)
                if all(_rejected(mut, q, k, v, fold, g, f"mutant [{name}] {fam} L={L} fold={fold} exact={exact}") for (fold, exact), g in gates.items()):
                    caught[name].append(fam)
        for name, fams_c in caught.items():
            report.append(f"L={L} H={H} [{name}] rejected by: {', '.join(fams_c) or 'NONE'}")
    print("\n".join(report))
    missed = [r for r in report if r.endswith("NONE")]
    assert not missed, "\n".join(missed)
