"""The masked attention gate of tests/attention_mask_ref.py discriminates, and flux_pipeline.build_region_groups builds the table its docstring
states.  CPU only.

Gate: the working-precision model passes it, and each listed mutant of the masked fp64 reference (rounded to bf16: a kernel wrong in that one
way and otherwise perfect) is rejected by at least one input family, under the gates of BOTH builds, at 1, 2, 6 and 51 key tiles."""
import pytest
import torch

import attention_mask_ref as mr
import attention_ref as ar
from parity_util import round_fp64_to_bf16

LENGTHS = [64, 100, 333, 3264]  # 1, 2, 6, 51 key tiles
FAMS = ("randn", "pos", "probe_last")


def _mutants(tab):
    """name -> the `allowed` matrix of a kernel that is wrong in one way.  The mutated keys lie among the last 128 (the probe's columns)."""
    L = tab.shape[-1]
    g, p = mr.split_desc(tab[0])
    allowed = mr.allowed_of(tab)
    out = {}
    j = L - 5  # a key of the last image band ("none" pattern, group 6): masked for the region text rows
    assert not allowed[0, :, j].all() and allowed[0, :, j].any()
    a = allowed.clone()
    a[0, :, j] = True
    out["one masked key admitted"] = a
    a = allowed.clone()
    a[0, :, j] = False
    a[0, j, j] = True
    out["one allowed key dropped"] = a
    g1 = torch.roll(g, 1)  # key j takes the group of key j - 1: every segment edge moves by one key
    out["key groups shifted by one"] = ((p[:, None] >> g1[None, :]) & 1).bool()[None]
    i1, i2 = int((g == 1).nonzero()[0]), L - 1  # a region-1 text row and an uncovered image row: their permission sets differ
    assert p[i1] != p[i2]
    p2 = p.clone()
    p2[i1], p2[i2] = p[i2], p[i1]
    out["two permission rows exchanged"] = ((p2[:, None] >> g[None, :]) & 1).bool()[None]
    return out


def _rejected(mut, q, k, v, fold, gate, what):
    try:
        ar.assert_attention_close(round_fp64_to_bf16(mut), q, k, v, fold, what, gate=gate)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("L", LENGTHS)
def test_masked_model_passes_and_mutants_fail(L):
    tab = mr.table_two_regions(L)[None]
    assert mr.self_admitting(tab)
    allowed = mr.allowed_of(tab)
    mutants = _mutants(tab)
    caught = {name: [] for name in mutants}
    for fam in FAMS:
        q, k, v = ar.attention_inputs(fam, 1, 1, L, seed=12)
        ref_A = mr.attention_ref64_masked(q, k, v, allowed)
        gates = {fold: mr.masked_gate(q, k, v, allowed, fold, ref_A=ref_A) for fold in (False, True)}
        for fold, g in gates.items():
            ar.assert_attention_close(mr.attention_model_masked(q, k, v, allowed, fold), q, k, v, fold, f"masked model {fam} L={L} fold={fold}", gate=g)
            assert g["r_model"] <= 1.1, f"{fam} L={L} fold={fold}: the model itself sits at {g['r_model']:.3f} x the bound"
        for name, a in mutants.items():
            mut = mr.attention_ref64_masked(q, k, v, a)[0]
            if all(_rejected(mut, q, k, v, fold, g, f"mutant [{name}] {fam} L={L} fold={fold}") for fold, g in gates.items()):
                caught[name].append(fam)
    report = [f"L={L} [{name}] rejected by: {', '.join(f) or 'NONE'}" for name, f in caught.items()]
    print("\n".join(report))
    missed = [r for r in report if r.endswith("NONE")]
    assert not missed, "\n".join(missed)


def test_masked_reference_is_sdpa_with_a_mask():
    """attention_ref64_masked == F.scaled_dot_product_attention(q, k, v, attn_mask=allowed) in fp64; the all-allowed table == the dense reference"""
    L = 97
    q, k, v = ar.attention_inputs("randn", 2, 2, L, seed=3)
    tab = torch.stack((mr.table_two_regions(L), mr.table_stripes(L)))
    allowed = mr.allowed_of(tab)
    ref, A = mr.attention_ref64_masked(q, k, v, allowed)
    sdpa = torch.nn.functional.scaled_dot_product_attention(q.double(), k.double(), v.double(), attn_mask=allowed[:, None])
    assert (ref - ar.to_rows(sdpa)).abs().max().item() <= 1e-13
    assert (ref.abs() <= A + 1e-300).all()
    dense = ar.attention_ref64(q, k, v)[0]
    full = mr.allowed_of(mr.table_all(L)[None].expand(2, L))
    assert torch.equal(mr.attention_ref64_masked(q, k, v, full)[0], dense)


def test_tables_are_self_admitting_and_shaped():
    for L in (64, 100, 333, 448, 3264):
        for fn in (mr.table_all, mr.table_first_tiles_masked, mr.table_last_tiles_masked, mr.table_stripes, mr.table_two_regions):
            t = fn(L)
            assert t.shape == (L,) and mr.self_admitting(t), f"{fn.__name__} L={L}"
            assert torch.equal(mr.to_i32(t).to(torch.int64) & 0xFFFFFFFF, t)
    # (b) / (c) really mask whole tiles for some rows
    a = mr.allowed_of(mr.table_first_tiles_masked(333))
    assert not a[-1, :128].any() and a[-1, 128:].all() and a[0].all()
    a = mr.allowed_of(mr.table_last_tiles_masked(333))
    assert not a[0, 205:].any() and a[0, :205].all() and a[-1].all()


# ---- build_region_groups ----------------------------------------------------------------------------------------------------------------
def _two_boxes(h=8, w=8):
    from flux_pipeline import region_token_grid

    ga = region_token_grid({"prompt": "a", "box": (0.0, 0.0, 0.6, 1.0)}, 16 * h, 16 * w)  # columns 0..4 (token 4 is covered to 0.8)
    gb = region_token_grid({"prompt": "b", "box": (0.5, 0.25, 1.0, 1.0)}, 16 * h, 16 * w)  # columns 4..7, rows 2..7
    return torch.stack((ga, gb))


def test_region_groups_on_two_overlapping_boxes():
    from flux_pipeline import build_region_groups

    grids = _two_boxes()
    assert grids[0].sum() == 8 * 5 and grids[1].sum() == 6 * 4
    nb, rt = 5, 16
    t = build_region_groups(nb, rt, grids)
    L = nb + 2 * rt + 64
    assert t.dtype == torch.int32 and t.shape == (L,)
    g, p = mr.split_desc(t)
    # key groups: 0 base, 1 / 2 region texts, then patterns ascending as bit sets: none (0) -> 3, {a} (1) -> 4, {b} (2) -> 5, {a, b} (3) -> 6
    assert (g[:nb] == 0).all() and (g[nb:nb + rt] == 1).all() and (g[nb + rt:nb + 2 * rt] == 2).all()
    img = g[nb + 2 * rt:].reshape(8, 8)
    want = torch.full((8, 8), 4)
    want[:, 5:] = 3
    want[2:, 5:] = 5
    want[2:, 4] = 6
    assert torch.equal(img, want)
    IMG = 0b1111000
    assert (p[:nb] == (1 | IMG)).all()                                # base text: group 0 + every image group
    assert (p[nb:nb + rt] == (0b10 | 1 << 4 | 1 << 6)).all()          # region a: itself + patterns {a}, {a, b}
    assert (p[nb + rt:nb + 2 * rt] == (0b100 | 1 << 5 | 1 << 6)).all()
    pi = p[nb + 2 * rt:].reshape(8, 8)
    assert pi[0, 0] == (1 | 0b010 | IMG) and pi[0, 7] == (1 | IMG) and pi[7, 7] == (1 | 0b100 | IMG) and pi[7, 4] == (1 | 0b110 | IMG)
    assert mr.self_admitting(t)
    a = mr.allowed_of(t)
    assert a[nb + 2 * rt:, nb + 2 * rt:].all(), "image-to-image attention stays dense"
    assert not a[nb, nb + rt] and not a[nb + rt, 0] and not a[0, nb], "the three texts do not see each other"
    # a Kontext reference: its rows carry the pattern `none`
    tr = build_region_groups(nb, rt, grids, n_ref=7)
    gr, pr = mr.split_desc(tr)
    assert tr.shape == (L + 7,) and (gr[-7:] == 3).all() and (pr[-7:] == (1 | IMG)).all() and torch.equal(tr[:L], t)


def test_region_groups_negative_branch():
    from flux_pipeline import build_region_groups

    nb, rt = 5, 16
    t = build_region_groups(nb, rt, _two_boxes(), negative=True)
    g, p = mr.split_desc(t)
    assert torch.equal(g, mr.split_desc(build_region_groups(nb, rt, _two_boxes()))[0]), "the key groups are those of the prompt branch"
    IMG = 0b1111000
    assert (p[:nb] == (1 | IMG)).all() and (p[nb:nb + rt] == 0b10).all() and (p[nb + rt:nb + 2 * rt] == 0b100).all()
    assert (p[nb + 2 * rt:] == (1 | IMG)).all(), "no image query sees a region text in the negative branch"
    assert mr.self_admitting(t)
    a = mr.allowed_of(t)
    assert not a[:nb, nb:nb + 2 * rt].any() and not a[nb + 2 * rt:, nb:nb + 2 * rt].any(), "the region rows are inert: nobody else reads them"


def test_region_groups_refusals():
    from flux_pipeline import build_region_groups, region_token_grid

    # 4 regions in general position need 1 + 4 + 2^4 groups
    ys, xs = torch.arange(8)[:, None], torch.arange(8)[None, :]
    many = torch.stack([((xs >> i) % 2 == 0).expand(8, 8) if i < 2 else ((ys >> (i - 2)) % 2 == 0).expand(8, 8) for i in range(4)])
    with pytest.raises(ValueError, match="attention groups"):
        build_region_groups(4, 16, many)
    with pytest.raises(ValueError, match="attention groups"):
        build_region_groups(4, 16, torch.ones(15, 2, 2, dtype=torch.bool))
    empty = torch.zeros(2, 4, 4, dtype=torch.bool)
    empty[0, 0, 0] = True
    with pytest.raises(ValueError, match="covers no image token"):
        build_region_groups(4, 16, empty)
    with pytest.raises(ValueError, match="covers no image token"):
        region_token_grid({"prompt": "x", "box": (0.0, 0.0, 0.02, 0.02)}, 128, 128)  # a third of a token
    with pytest.raises(ValueError, match="exactly one of"):
        region_token_grid({"prompt": "x"}, 128, 128)
    with pytest.raises(ValueError, match="box"):
        region_token_grid({"prompt": "x", "box": (0.5, 0.0, 0.2, 1.0)}, 128, 128)
    # a mask image: area-averaged to the token grid, thresholded at 0.5
    m = torch.zeros(64, 64, dtype=torch.uint8)
    m[:, :20] = 255  # 64 px -> 4 tokens of 16 px: token 0 fully, token 1 to 4 / 16
    assert torch.equal(region_token_grid({"prompt": "x", "mask": m}, 64, 64), torch.tensor([[True, False, False, False]] * 4))


def test_every_token_admits_itself_on_random_layouts():
    from flux_pipeline import build_region_groups

    g = torch.Generator().manual_seed(4)
    for _ in range(20):
        R = int(torch.randint(1, 4, (1,), generator=g))
        grids = torch.rand(R, 6, 7, generator=g) < 0.5
        grids[:, 0, 0] = True
        for neg in (False, True):
            t = build_region_groups(int(torch.randint(0, 40, (1,), generator=g)), 16, grids, n_ref=int(torch.randint(0, 9, (1,), generator=g)), negative=neg)
            assert mr.self_admitting(t)
            assert int(mr.split_desc(t)[0].max()) < 16


def test_region_mask_value_ranges():
    """the same left-half mask as 0 / 255 bytes, 0 / 1 bytes (what a bilevel image decodes to), bool, 0..1 floats, and PIL images of
    modes L and 1 (and a PNG of mode 1 passed as a path): one grid"""
    import numpy as np
    from PIL import Image

    from flux_pipeline import region_token_grid

    m = torch.zeros(64, 128, dtype=torch.uint8)
    m[:, :64] = 255
    want = torch.zeros(4, 8, dtype=torch.bool)
    want[:, :4] = True
    bilevel = Image.fromarray(m.numpy()).convert("1")
    forms = [m, m // 255, m.bool(), m.float() / 255, m.numpy(), (m // 255).numpy(), m.bool().numpy(), Image.fromarray(m.numpy()), bilevel,
             torch.from_numpy(np.array(bilevel)).type(torch.uint8)]  # the last: what load_init_image_if_needed makes of a bilevel file
    for f in forms:
        assert torch.equal(region_token_grid({"prompt": "a", "mask": f}, 64, 128), want), type(f)
