"""CPU: the LyCORIS side of lora_loading.py (key recognition, scale rule, refusals) and the restatement that tests/test_adapter_fuse_gpu.py
holds the kernel to: its deltas equal the textbook forms in fp64, and on every GPU case its fp32-sum form meets the GPU gates against its
fp64 form (the seeds leave the amax off a bf16 tie and the gates room for nothing but the summation order)."""
import warnings

import pytest
import torch

import test_adapter_fuse_gpu as tg

P = "lora_unet_double_blocks_3_txt_mlp_2"
Z = torch.zeros


def adapter(leaves):
    import lora_loading as ll

    keys, sd = ll.resolve_lora_state_dict({f"{P}.{k}": v for k, v in leaves.items()})
    assert keys == ["double_blocks.3.txt_mlp.2"], keys
    return ll.get_adapter_for_key(keys[0], sd)


@pytest.mark.parametrize("leaves,kind,scale,shapes", [
    (dict(hada_w1_a=Z(8, 2), hada_w1_b=Z(2, 6), hada_w2_a=Z(8, 2), hada_w2_b=Z(2, 6), alpha=torch.tensor(3.0)), "loha", 1.5, [(8, 2), (2, 6)] * 2),
    (dict(hada_w1_a=Z(8, 2), hada_w1_b=Z(2, 6), hada_w2_a=Z(8, 2), hada_w2_b=Z(2, 6)), "loha", 1.0, [(8, 2), (2, 6)] * 2),
    (dict(lokr_w1=Z(2, 3), lokr_w2=Z(4, 2), alpha=torch.tensor(3.0)), "lokr", 1.0, [(2, 3), (4, 2)]),  # both factors full: no rank, scale 1
    (dict(lokr_w1=Z(2, 3), lokr_w2_a=Z(4, 5), lokr_w2_b=Z(5, 2), alpha=torch.tensor(2.5)), "lokr", 0.5, [(2, 3), (4, 2)]),
    (dict(lokr_w1_a=Z(2, 4), lokr_w1_b=Z(4, 3), lokr_w2=Z(4, 2), alpha=torch.tensor(2.0), dora_scale=Z(8)), "lokr", 0.5, [(2, 3), (4, 2)]),
    (dict(diff=Z(8, 6), alpha=torch.tensor(9.0)), "full", 1.0, [(8, 6)]),
    ({"lora_down.weight": Z(2, 6), "lora_up.weight": Z(8, 2), "alpha": torch.tensor(1.0)}, "lora", 1.0, [(8, 2), (2, 6)]),
], ids=["loha", "loha-no-alpha", "lokr-full", "lokr-w2-decomposed", "lokr-w1-decomposed-dora", "diff", "lora"])
def test_key_layouts_and_scale_rule(leaves, kind, scale, shapes):
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        d = adapter(leaves)
    assert (d.kind, d.scale, [tuple(f.shape) for f in d.factors]) == (kind, scale, shapes)
    assert [("dora_scale" in str(w.message)) for w in seen] == ([True] if "dora_scale" in leaves else [])


@pytest.mark.parametrize("leaf", ["hada_t1", "lokr_t2", "diff_b"])
def test_tucker_and_bias_deltas_are_refused_by_name(leaf):
    with pytest.raises(ValueError, match=leaf):
        adapter({leaf: Z(2, 2), "diff": Z(8, 6)})


@pytest.mark.parametrize("kind,kw", tg.CASES + [("mixed", {})], ids=str)
@pytest.mark.parametrize("N,K", tg.SHAPES)
def test_restatement_and_seeds(kind, kw, N, K):
    q8, recip, terms = tg.mixed_inputs() if kind == "mixed" else tg.case_inputs(kind, kw, N, K)
    w = q8.double() * recip.double()
    for t in terms:  # the textbook forms (Delta.dense restates them in fp32 for un-quantised layers)
        f = [x.double() for x in t.factors]
        ref = {"lora": lambda: sum(f[0] @ c for c in f[1].chunk(t.n_chunks, 0)), "loha": lambda: (f[0] @ f[1]) * (f[2] @ f[3]),
               "lokr": lambda: torch.kron(f[0], f[1]), "full": lambda: f[0]}[t.kind]() * float(torch.tensor(t.scale, dtype=torch.float32))
        w = w + ref
        assert torch.allclose(t.dense().double(), ref, rtol=1e-4, atol=1e-6)
    got, exact = tg.restate(q8, recip, terms), tg.restate(q8, recip, terms, fp64=True)
    tg.gate(got, exact, kind in ("lokr", "full"), f"fp32 vs fp64 restatement {kind} {kw} {N}x{K}")
    assert (tg.fo.quantize_weight(w.float().bfloat16())[0].view(torch.uint8) != exact[0]).double().mean() < 1e-3  # and both say what the textbook says
    assert w.abs().max() > 0.62, "the deltas did not move the amax (the weight alone reaches 0.606)"
