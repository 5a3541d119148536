"""CPU: the restatement tests/test_dora_fuse_gpu.py holds the DoRA kernel to, and the loader's reading of `dora_scale`.  On every GPU case the
fp32-sum restatement meets the GPU gates against the fp64 one: the seeds leave the amax off a bf16 tie, so the bit-identical-scale gate is
fair and leaves room for the summation order and nothing else.  If a seed fails here, change the seed, not the gate."""
import pytest
import torch

import test_adapter_fuse_gpu as tg
import test_dora_fuse_gpu as td


@pytest.mark.parametrize("s", [1.0, 0.6])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("N,K", tg.SHAPES)
@pytest.mark.parametrize("kind,kw", td.KINDS + [(td.THREE, None)], ids=td.ids)
def test_restatement_seeds_and_the_magnitude_matters(kind, kw, N, K, axis, s):
    q8, recip, terms, m = td.case_inputs(kind, kw, N, K, axis)
    (exact, fac), (got, _) = td.restate_apply(q8, recip, terms, m, axis, s, fp64=True), td.restate_apply(q8, recip, terms, m, axis, s)
    tg.gate(got, exact, False, f"fp32 vs fp64 restatement {kind} {kw} {N}x{K} axis {axis} s {s}")
    plain = tg.restate(q8, recip, terms, fp64=True)[0]
    assert (plain != exact[0]).double().mean() > 0.10, "the magnitude changed next to nothing: a kernel that ignored it could pass"
    if s == 0.6:  # (at s = 1 the zero magnitude leaves a_i = 0, which has no inverse) REMOVE on the APPLY result, both sums
        a8 = exact[0].view(torch.float8_e4m3fn)
        tg.gate(td.restate_remove(a8, exact[2], terms, fac, axis), td.restate_remove(a8, exact[2], terms, fac, axis, fp64=True), False, "remove")


@pytest.mark.parametrize("shape,axis", [((8, 1), 0), ((8,), 0), ((1, 6), 1), ((6,), None), ((3, 5), None), ((1, 8), None)], ids=str)
def test_dora_scale_shapes(shape, axis):
    import lora_loading as ll

    P, key = "lora_unet_double_blocks_3_txt_mlp_2", "double_blocks.3.txt_mlp.2"
    sd = ll.resolve_lora_state_dict({f"{P}.lora_down.weight": torch.ones(2, 6), f"{P}.lora_up.weight": torch.ones(8, 2), f"{P}.dora_scale": torch.rand(shape)})[1]
    if axis is None:
        with pytest.raises(ValueError, match=r"dora_scale.*" + str(list(shape)).replace("[", r"\[")):
            ll.get_dora_for_key(key, sd, 8, 6)
        return
    d, m, got = ll.get_dora_for_key(key, sd, 8, 6)
    assert (d.kind, got, tuple(m.shape)) == ("lora", axis, ((8, 6)[axis],)) and torch.equal(m, sd[f"{key}.dora_scale"].reshape(-1))
    assert ll.get_dora_for_key(key, {k: v for k, v in sd.items() if "dora" not in k}, 8, 6)[1:] == (None, None)
    sq = {f"{key}.lora_A.weight": torch.ones(2, 8), f"{key}.lora_B.weight": torch.ones(8, 2), f"{key}.dora_scale": torch.ones(8)}
    assert ll.get_dora_for_key(key, sq, 8, 8)[2] == 0  # 1-D with N == K: the output axis
