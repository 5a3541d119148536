"""fluxmi_adapter_fuse_dora_f8 (csrc/adapter_fuse.hip) and the DoRA side of the loader against a torch restatement of include/fluxmi.h's
arithmetic with the rank products and norm sums in fp64, rounded once to fp32, under test_adapter_fuse_gpu.gate (scale pair bit-identical, no
byte more than one e4m3 code off, >= 99.9 % identical).  tests/test_dora_cpu.py holds the fp32-sum restatement to the same gates: the seeds."""
import warnings

import pytest
import torch
from torch import nn

import test_adapter_fuse_gpu as tg
from parity_util import f8_ord

KINDS = [("lora", dict(rank=1)), ("lora", dict(rank=17)), ("loha", dict(rank=17)), ("lokr", dict(block=(24, 16))), ("full", {})]
THREE = [("lora", dict(rank=17)), ("lokr", dict(block=(24, 16))), ("full", {})]
PAD, MARK = 1024, 12345.0  # floats of sentinel around factors and work
ids = lambda v: v if isinstance(v, str) else "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else None


def delta(terms, fp64):
    """D = d_0, D = fl(D + d_t): the (single-chunk) deltas of test_adapter_fuse_gpu.restate, summed apart from the weight"""
    mm = (lambda a, b: (a.double() @ b.double()).float()) if fp64 else (lambda a, b: a @ b)
    D = None
    for t in terms:
        f = t.factors
        d = {"lora": lambda: mm(f[0], f[1]), "loha": lambda: mm(f[0], f[1]) * mm(f[2], f[3]), "lokr": lambda: torch.kron(f[0], f[1]), "full": lambda: f[0]}[t.kind]()
        d = d * torch.tensor(t.scale, dtype=torch.float32)
        D = d if D is None else D + d
    return D


def rescale(q8, recip, terms, a, b, axis, fp64):
    w, D = q8.float() * recip, delta(terms, fp64)
    q, s, r = tg.fo.quantize_weight(((a.unsqueeze(1 - axis) * w) + (b.unsqueeze(1 - axis) * D)).bfloat16())
    return q.view(torch.uint8), s, r


def restate_apply(q8, recip, terms, m, axis, s, fp64=False):
    """include/fluxmi.h's APPLY on the CPU -> ((bytes, scale, recip), factors [2, N or K])"""
    v, s = q8.float() * recip + delta(terms, fp64), torch.tensor(s, dtype=torch.float32)
    ss = (v.double() ** 2).sum(1 - axis) if fp64 else (v * v).sum(1 - axis).double()
    b = s * (m / (ss.sqrt().float() + 2.0 ** -23))
    return rescale(q8, recip, terms, (1 - s) + b, b, axis, fp64), torch.stack([(1 - s) + b, b])


def restate_remove(q8, recip, terms, factors, axis, fp64=False):
    return rescale(q8, recip, terms, 1 / factors[0], -(factors[1] / factors[0]), axis, fp64)


def case_inputs(kind, kw, N, K, axis):
    """test_adapter_fuse_gpu's weight and term(s); a magnitude |w row / column| * (1 + 0.2 randn) with a few negative and one zero entry"""
    q8, recip, g = tg.make_weight(N, K, 1000 + N)
    terms = [tg.make_term(k, N, K, g, **w) for k, w in (kind if isinstance(kind, list) else [(kind, kw)])]
    m = (q8.float() * recip).norm(dim=1 - axis) * (1 + 0.2 * torch.randn((N, K)[axis], generator=g))
    m[1::17] *= -1
    m[3] = 0.0
    return q8, recip, terms, m


def dora_on_gpu(dev, q8, recip, terms, m, axis, s, factors=None):
    """one C call with the weight, factors and work each inside a sentinel frame -> ((bytes, scale, recip), factors); asserts the frames"""
    from fluxmi import _lib, ops

    N, K = q8.shape
    wbuf = torch.full((2 * tg.FRAME + N * K,), tg.SENTINEL, dtype=torch.uint8, device=dev)
    w = wbuf[tg.FRAME:tg.FRAME + N * K]
    w.copy_(q8.view(torch.uint8).reshape(-1))
    n_work = _lib.lib.fluxmi_adapter_dora_work_bytes(N, K, axis) // 4
    assert n_work == (N * -(-K // 128) if axis == 0 else -(-N // 128) * K)
    fbuf, kbuf = torch.full((2 * PAD + 2 * (N, K)[axis],), MARK, device=dev), torch.full((2 * PAD + n_work,), MARK, device=dev)
    if factors is not None:
        fbuf[PAD:-PAD].copy_(factors.reshape(-1))
    sc, rc, tmp, mag = (1 / recip).to(dev), recip.clone().to(dev), torch.empty(4, device=dev), None if m is None else m.to(dev)
    arr, keep = ops.delta_terms(terms, N, K, dev)
    _lib.call("fluxmi_adapter_fuse_dora_f8", w.data_ptr(), sc.data_ptr(), rc.data_ptr(), arr, len(terms), N, K, axis, None if mag is None else mag.data_ptr(),
              float(s), _lib.DORA_APPLY if factors is None else _lib.DORA_REMOVE, fbuf[PAD:].data_ptr(), kbuf[PAD:].data_ptr(), tmp.data_ptr(), None)
    out = wbuf.cpu()
    assert bool((out[:tg.FRAME] == tg.SENTINEL).all()) and bool((out[tg.FRAME + N * K:] == tg.SENTINEL).all()), "bytes outside [0, N * K) were written"
    assert all(bool((b[:PAD] == MARK).all()) and bool((b[-PAD:] == MARK).all()) for b in (fbuf, kbuf)), "floats outside factors or work were written"
    return (out[tg.FRAME:tg.FRAME + N * K].view(N, K), sc.cpu(), rc.cpu()), fbuf[PAD:-PAD].cpu().view(2, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("s", [1.0, 0.6])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("N,K", tg.SHAPES)
@pytest.mark.parametrize("kind,kw", KINDS, ids=ids)
def test_kinds_axes_and_strengths(dev, kind, kw, N, K, axis, s):
    q8, recip, terms, m = case_inputs(kind, kw, N, K, axis)
    got, fac = dora_on_gpu(dev, q8, recip, terms, m, axis, s)
    exp, efac = restate_apply(q8, recip, terms, m, axis, s, fp64=True)
    assert torch.allclose(fac, efac, rtol=1e-6, atol=1e-7), "factors"  # (a few fp32 ulps of n_i, of a_i where (1 - s) + b_i cancels)
    tg.gate(got, exp, False, f"dora {kind} {kw} {N}x{K} axis {axis} s {s}")


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [0, 1])
def test_remove_inverts_apply(dev, axis):
    """REMOVE on the GPU's own post-APPLY bytes and factors against its restatement, under the same gates.  Then the round trip on a weight
    and an adapter of a trained model's proportions: Gaussian weights, a delta of 1 % of their size, magnitudes within 2 % of the norm.  An
    element comes back within one code when the fp8 rounding of w' = a (w + D) (at most 2^-4 of it) stays under one and a half steps of w
    (2^-4 .. 2^-3 of it), which |D| < |w| / 2 guarantees; a Gaussian w is that small in about 1.3 |D| / sigma = 1.3 % of the elements at
    the very worst, and the bound asked for is 99 %."""
    q8, recip, terms, m = case_inputs("lora", dict(rank=17), 200, 208, axis)
    applied, fac = dora_on_gpu(dev, q8, recip, terms, m, axis, 0.6)
    a8 = applied[0].view(torch.float8_e4m3fn)
    tg.gate(dora_on_gpu(dev, a8, applied[2], terms, None, axis, 0.6, fac)[0], restate_remove(a8, applied[2], terms, fac, axis, fp64=True), False, f"remove axis {axis}")
    g = torch.Generator().manual_seed(9 + axis)
    q8, _, recip = tg.fo.quantize_weight((torch.randn(200, 208, generator=g) * 0.05).bfloat16())
    term = tg.make_term("lora", 200, 208, g, rank=17, amp=0.0005)
    m = ((q8.float() * recip) + term.dense()).norm(dim=1 - axis) * (1 + 0.02 * torch.randn((200, 208)[axis], generator=g))
    applied, fac = dora_on_gpu(dev, q8, recip, [term], m, axis, 1.0)
    back = dora_on_gpu(dev, applied[0].view(torch.float8_e4m3fn), applied[2], [term], None, axis, 1.0, fac)[0]
    share = ((f8_ord(back[0]) - f8_ord(q8.view(torch.uint8))).abs() <= 1).double().mean().item()
    print(f"round trip axis {axis}: {share:.6f} of the original bytes within one code")
    assert share >= 0.99 and not torch.equal(applied[0], q8.view(torch.uint8))


@pytest.mark.gpu
def test_three_terms_one_magnitude_through_the_op(dev):
    from fluxmi import ops

    q8, recip, terms, m = case_inputs(THREE, None, 200, 208, 0)
    runs = []
    for _ in range(2):
        w, sc, rc = q8.clone().to(dev), (1 / recip).to(dev), recip.clone().to(dev)
        fac = ops.adapter_fuse_dora_f8(w, sc, rc, terms, m, axis=0, strength=0.6)
        runs.append((w.cpu().view(torch.uint8), sc.cpu(), rc.cpu(), fac.cpu()))
    assert all(torch.equal(x, y) for x, y in zip(*runs)), "the same inputs gave other bytes or factors"
    tg.gate(runs[0][:3], restate_apply(q8, recip, terms, m, 0, 0.6, fp64=True)[0], False, "three terms, one magnitude")


@pytest.mark.gpu
@pytest.mark.parametrize("text,bad", [("axis", dict(axis=2)), ("magnitude", dict(magnitude=None)), ("mode", dict(mode=2)), ("strength", dict(strength=float("nan"))),
                                      ("K % 16", dict(K=72))], ids=str)
def test_refusals_write_nothing(dev, text, bad):
    from fluxmi import _lib

    N, K = 48, bad.get("K", 64)
    w = torch.full((N * K,), tg.SENTINEL, dtype=torch.uint8, device=dev)
    st = torch.full((6 + 2 * 128 + 128 * 128,), 3.0, device=dev)  # scale, recip, amax_tmp, factors, work
    f = torch.zeros(128 * 128, device=dev)
    arr = (_lib.DeltaTerm * 1)(_lib.DeltaTerm(kind=0, rank=4, n_chunks=1, scale=1.0, p0=f.data_ptr(), p1=f.data_ptr()))
    kw = {**dict(axis=0, magnitude=f.data_ptr(), mode=0, strength=1.0), **bad}
    rc = _lib.lib.fluxmi_adapter_fuse_dora_f8(w.data_ptr(), st[0:1].data_ptr(), st[1:2].data_ptr(), arr, 1, N, K, kw["axis"], kw["magnitude"], kw["strength"],
                                              kw["mode"], st[6:].data_ptr(), st[6 + 256:].data_ptr(), st[2:6].data_ptr(), None)
    torch.cuda.synchronize()
    assert rc != 0 and text in _lib.lib.fluxmi_last_error().decode(), _lib.lib.fluxmi_last_error()
    assert bool((w == tg.SENTINEL).all()) and bool((st == 3.0).all())


# ---- the loader: a kohya-keyed DoRA dict into two F8Linear modules and one nn.Linear, through Flux's own load / unload bookkeeping ----------
QKV, PROJ = "double_blocks.0.img_attn.qkv", "double_blocks.0.img_attn.proj"


def toy_model(dev):
    from modules.flux_model import Flux

    class Toy(nn.Module):
        get_lora, has_lora, load_lora, unload_lora = Flux.get_lora, Flux.has_lora, Flux.load_lora, Flux.unload_lora
        rebind_weights = lambda self: None

    model = Toy()
    model.double_blocks, model.loras = tg.toy_model(dev).double_blocks, []
    model.double_blocks[0].img_mod = nn.Module()
    model.double_blocks[0].img_mod.lin = nn.Linear(64, 32, bias=False, device=dev)
    return model


def toy_adapter(dora=True):
    """rank-4 LoRA on qkv (dora_scale [N, 1]), proj (dora_scale [1, K]) and img_mod.lin (none) -> (resolved dict, {module: (Delta, magnitude, axis)})"""
    import lora_loading as ll
    from fluxmi import ops

    g = torch.Generator().manual_seed(31)
    sd, want = {}, {}
    for name, (n, k), axis in ((QKV, (96, 64), 0), (PROJ, (48, 64), 1), ("double_blocks.0.img_mod.lin", (32, 64), None)):
        up, down = torch.randn(n, 4, generator=g) * 0.05, torch.randn(4, k, generator=g) * 0.05
        m = None if axis is None or not dora else 0.4 * (1 + 0.2 * torch.randn((n, k)[axis], generator=g))
        p = "lora_unet_" + name.replace(".", "_")
        sd.update({f"{p}.lora_up.weight": up, f"{p}.lora_down.weight": down, f"{p}.alpha": torch.tensor(2.0)})
        if m is not None:
            sd[f"{p}.dora_scale"] = m.unsqueeze(1 - axis)
        want[name] = (ops.Delta("lora", (up, down * 2.0 / 4)), m, axis)
    return ll.resolve_lora_state_dict(sd)[1], want


def toy_state(model):
    b = model.double_blocks[0]
    f8 = {n: (m.float8_data.cpu().view(torch.uint8).clone(), m.scale.cpu().clone(), m.scale_reciprocal.cpu().clone()) for n, m in ((QKV, b.img_attn.qkv), (PROJ, b.img_attn.proj))}
    return f8, b.img_mod.lin.weight.detach().float().cpu().clone()


@pytest.mark.gpu
def test_loader_dora_load_unload_and_order(dev):
    model = toy_model(dev)
    sd, want = toy_adapter()
    before, lin0 = toy_state(model)
    same = lambda x, y: all(torch.equal(p, q) for n in x for p, q in zip(x[n], y[n]))
    with pytest.raises(ValueError, match=r"qkv\.dora_scale.*\[3, 5\]"):  # refused by name, nothing touched
        model.load_lora({**sd, f"{QKV}.dora_scale": torch.ones(3, 5)}, 1.0, name="odd")
    assert same(before, toy_state(model)[0]) and model.loras == []
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no dora_scale warning on the fuse path
        model.load_lora(sd, 0.8, name="dora")
    after, lin1 = toy_state(model)
    record = model.get_lora("dora")
    for key in (QKV, PROJ):
        d, m, axis = want[key]
        tg.gate(after[key], restate_apply(before[key][0].view(torch.float8_e4m3fn), before[key][2], [d], m, axis, 0.8, fp64=True)[0], False, f"load {key}")
        assert record.dora[key][1] == axis and tuple(record.dora[key][0].shape) == (2, before[key][0].shape[axis])
    assert torch.allclose(lin1, lin0 + 0.8 * want["double_blocks.0.img_mod.lin"][0].dense(), rtol=0, atol=2e-7)  # fp32 weight, no magnitude: plain LoRA

    model.load_lora(toy_adapter(dora=False)[0], 0.5, name="plain")
    held = toy_state(model)[0]
    with pytest.raises(ValueError, match="plain"):  # DoRA does not commute with the later fuse
        model.unload_lora("dora")
    assert same(held, toy_state(model)[0]) and len(model.loras) == 2
    model.unload_lora("plain")
    start, factors = toy_state(model)[0], {k: v[0].cpu() for k, v in record.dora.items()}
    assert model.unload_lora("dora") and model.loras == []
    end, lin2 = toy_state(model)
    for key in (QKV, PROJ):
        tg.gate(end[key], restate_remove(start[key][0].view(torch.float8_e4m3fn), start[key][2], [want[key][0]], factors[key], want[key][2], fp64=True), False, f"unload {key}")
    assert torch.allclose(lin2, lin0, rtol=0, atol=1e-6)
