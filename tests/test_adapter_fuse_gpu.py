"""fluxmi_adapter_fuse_f8 (csrc/adapter_fuse.hip) and the LyCORIS loader against a plain torch restatement of the arithmetic stated in
include/fluxmi.h.  LoKr and full deltas involve no summation: bytes, scale and reciprocal are bit-identical.  LoRA and LoHa are held to the
restatement with the rank products in fp64, rounded once to fp32, under the LoRA-fuse gates of DESIGN.md's config-5 row: scale bit-identical,
>= 99.9 % of the bytes identical, no byte more than one e4m3 code off.  tests/test_adapters_cpu.py checks that the fp32-sum restatement
meets the same gates on every case here (the seeds), so the gates leave room for the summation order and nothing else."""
import pytest
import torch
from torch import nn

import flux_oracle as fo
from parity_util import f8_ord

SHAPES = [(48, 64), (200, 208), (384, 320)]  # none a multiple of the 128 x 128 tile; the first narrower than a tile both ways
FRAME, SENTINEL = 4096, 0x5B
CASES = ([("lora", dict(rank=r)) for r in (1, 17, 128)] + [("lora", dict(rank=17, n_chunks=3))] + [("loha", dict(rank=r)) for r in (1, 17, 128)]
         + [("lokr", dict(block=b)) for b in ((24, 16), "full", (1, 1))] + [("full", {})])


def make_weight(N, K, seed):
    """random e4m3 bytes (no NaN code) with zeros of both signs and the largest finite code planted; values up to 448 * recip = 0.6"""
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(0, 256, (N, K), generator=g, dtype=torch.int32)
    b = torch.where((b & 0x7F) == 0x7F, 0, b).to(torch.uint8)
    b[0, :4] = torch.tensor([0x00, 0x80, 0x7E, 0xFE], dtype=torch.uint8)
    return b.view(torch.float8_e4m3fn), torch.tensor(0.6 / 448 * 1.01, dtype=torch.float32), g


def make_term(kind, N, K, g, rank=4, n_chunks=1, block=None, amp=0.3):
    """a Delta whose elements are about `amp` in size: the sum moves the amax of a weight of amplitude 0.6"""
    from fluxmi import ops

    rn = lambda *s: torch.randn(*s, generator=g)
    if kind == "lora":
        return ops.Delta("lora", (rn(N, rank), rn(n_chunks * rank, K)), amp / (rank * n_chunks) ** 0.5, n_chunks)
    if kind == "loha":
        return ops.Delta("loha", (rn(N, rank), rn(rank, K), rn(N, rank), rn(rank, K)), amp / rank)
    if kind == "lokr":
        kn, kk = (N, K) if block == "full" else block
        kn = kn if N % kn == 0 else kn + 1  # (24, 16) -> (25, 16) at N = 200, which 24 does not divide: block edges still fall inside a tile
        return ops.Delta("lokr", (rn(N // kn, K // kk), rn(kn, kk)), amp)
    return ops.Delta("full", (rn(N, K),), amp)


def restate(q8, recip, terms, fp64=False):
    """include/fluxmi.h's arithmetic in torch on the CPU -> (bytes, scale, recip).  fp64: rank products in fp64, rounded once to fp32."""
    mm = (lambda a, b: (a.double() @ b.double()).float()) if fp64 else (lambda a, b: a @ b)
    acc = q8.float() * recip
    for t in terms:
        f, s = t.factors, torch.tensor(t.scale, dtype=torch.float32)
        if t.kind == "lora":
            ds = [mm(f[0], a) * s for a in f[1].chunk(t.n_chunks, 0)]
            d = ds[0] if len(ds) == 1 else sum(ds, torch.zeros_like(acc))
        elif t.kind == "loha":
            d = (mm(f[0], f[1]) * mm(f[2], f[3])) * s
        else:
            d = (torch.kron(f[0], f[1]) if t.kind == "lokr" else f[0]) * s
        acc = acc + d
    q, s, r = fo.quantize_weight(acc.bfloat16())
    return q.view(torch.uint8), s, r


def gate(got, exp, exact, what):
    (gq, gs, gr), (eq, es, er) = got, exp
    assert gs.view(torch.int32) == es.view(torch.int32) and gr.view(torch.int32) == er.view(torch.int32), f"{what}: scale {gs.item()!r} vs {es.item()!r}"
    d = (f8_ord(gq) - f8_ord(eq)).abs()
    same = (d == 0).double().mean().item()
    print(f"{what}: {same:.6f} of the bytes identical, largest difference {int(d.max())} codes")
    assert int(d.max()) <= (0 if exact else 1) and same >= (1.0 if exact else 0.999), what


def fuse_on_gpu(dev, q8, recip, calls):
    """runs each list of terms in `calls` as one op call on a window of a sentinel-filled buffer; asserts the frame around it is untouched"""
    from fluxmi import ops

    N, K = q8.shape
    buf = torch.full((2 * FRAME + N * K,), SENTINEL, dtype=torch.uint8, device=dev)
    w = buf[FRAME:FRAME + N * K].view(N, K)
    w.copy_(q8.view(torch.uint8))
    sc, rc = (1 / recip).to(dev), recip.clone().to(dev)
    for terms in calls:
        ops.adapter_fuse_f8(w.view(torch.float8_e4m3fn), sc, rc, terms)
    out = buf.cpu()
    assert bool((out[:FRAME] == SENTINEL).all()) and bool((out[FRAME + N * K:] == SENTINEL).all()), "bytes outside [0, N * K) were written"
    return out[FRAME:FRAME + N * K].view(N, K), sc.cpu(), rc.cpu()


def case_inputs(kind, kw, N, K):
    q8, recip, g = make_weight(N, K, 1000 + N)
    return q8, recip, [make_term(kind, N, K, g, **kw)]


def mixed_inputs(N=200, K=208):
    q8, recip, g = make_weight(N, K, 77)
    return q8, recip, [make_term(k, N, K, g, **kw) for k, kw in (("lora", dict(rank=17, n_chunks=3)), ("loha", dict(rank=9)), ("lokr", dict(block=(25, 16))))]


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("kind,kw", CASES, ids=lambda v: v if isinstance(v, str) else "-".join(f"{k}{x}" for k, x in v.items()))
def test_kinds_and_edge_shapes(dev, kind, kw, N, K):
    q8, recip, terms = case_inputs(kind, kw, N, K)
    exact = kind in ("lokr", "full")
    gate(fuse_on_gpu(dev, q8, recip, [terms]), restate(q8, recip, terms, fp64=not exact), exact, f"{kind} {kw} {N}x{K}")


@pytest.mark.gpu
@pytest.mark.parametrize("n_chunks", [1, 3])
def test_single_lora_term_equals_the_old_path(dev, n_chunks):
    from fluxmi import ops

    q8, recip, (t,) = case_inputs("lora", dict(rank=16, n_chunks=n_chunks), 200, 208)
    old, sc, rc = q8.clone().to(dev), (1 / recip).to(dev), recip.clone().to(dev)
    ops.lora_fuse_f8(old, sc, rc, t.factors[0].to(dev), t.factors[1].to(dev), t.scale, n_chunks=n_chunks)
    gate(fuse_on_gpu(dev, q8, recip, [[t]]), (old.cpu().view(torch.uint8), sc.cpu(), rc.cpu()), False, f"old path, {n_chunks} chunks")


@pytest.mark.gpu
def test_three_terms_in_one_call_and_one_at_a_time(dev):
    q8, recip, terms = mixed_inputs()
    gate(fuse_on_gpu(dev, q8, recip, [terms]), restate(q8, recip, terms, fp64=True), False, "three terms, one call")
    exp = (q8, None, recip)
    for t in terms:  # in place, call after call: each reads the bytes and the reciprocal the one before wrote
        exp = restate(exp[0].view(torch.float8_e4m3fn), exp[2], [t], fp64=True)
    gate(fuse_on_gpu(dev, q8, recip, [[t] for t in terms]), exp, False, "three terms, three calls")


REFUSALS = [("n_terms", dict(n_terms=0)), ("n_terms", dict(n_terms=9)), ("rank", dict(rank=0)), ("rank", dict(rank=129)), ("LOKR", dict(kind=2, kn=7, kk=16)),
            ("LOKR", dict(kind=2, kn=8, kk=5)), ("K % 16", dict(K=72)), ("null factor pointer", dict(p1=None)), ("unknown kind", dict(kind=4))]


@pytest.mark.gpu
@pytest.mark.parametrize("text,bad", REFUSALS, ids=str)
def test_refusals_write_nothing(dev, text, bad):
    from fluxmi import _lib

    N, K = 48, bad.get("K", 64)
    w = torch.full((N * K,), SENTINEL, dtype=torch.uint8, device=dev)
    st = torch.full((6,), 3.0, device=dev)
    f = torch.zeros(128 * 128, device=dev)
    t = _lib.DeltaTerm(kind=0, rank=4, n_chunks=1, kn=8, kk=16, scale=1.0, p0=f.data_ptr(), p1=f.data_ptr(), p2=f.data_ptr(), p3=f.data_ptr())
    for k, v in bad.items():
        if k not in ("n_terms", "K"):
            setattr(t, k, v)
    arr = (_lib.DeltaTerm * 9)(*[t] * 9)
    rc = _lib.lib.fluxmi_adapter_fuse_f8(w.data_ptr(), st[0:1].data_ptr(), st[1:2].data_ptr(), arr, bad.get("n_terms", 1), N, K, st[2:].data_ptr(), None)
    torch.cuda.synchronize()
    assert rc != 0 and text in _lib.lib.fluxmi_last_error().decode(), _lib.lib.fluxmi_last_error()
    assert bool((w == SENTINEL).all()) and bool((st == 3.0).all())


# ---- the loader: kohya-keyed LyCORIS dicts into a two-layer F8Linear model -----------------------------------------------------------------
def toy_model(dev, seed=5):
    from float8_quantize import F8Linear

    g = torch.Generator().manual_seed(seed)
    attn = nn.Module()
    for name, (n, k) in (("qkv", (96, 64)), ("proj", (48, 64))):
        lin = F8Linear(k, n, bias=False, device=dev, dtype=torch.bfloat16, float_weight=(torch.randn(n, k, generator=g) * 0.05).bfloat16().to(dev))
        lin.quantize_weight()
        setattr(attn, name, lin)
    block, model = nn.Module(), nn.Module()
    block.img_attn = attn
    model.double_blocks = nn.ModuleList([block])
    return model


def toy_adapter(seed):
    """qkv: LoHa (rank 3) in file A, plain LoRA in file B; proj: LoKr with a decomposed w2 -> (kohya-keyed dict, {layer: Delta at adapter scale 1})"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g) * 0.3
    p, sd, want = "lora_unet_double_blocks_0_img_attn_", {}, {}
    if seed % 2:
        f = (rn(96, 3), rn(3, 64), rn(96, 3), rn(3, 64))
        sd.update({f"{p}qkv.hada_w1_a": f[0], f"{p}qkv.hada_w1_b": f[1], f"{p}qkv.hada_w2_a": f[2], f"{p}qkv.hada_w2_b": f[3], f"{p}qkv.alpha": torch.tensor(1.5)})
        want["qkv"] = ("loha", f, 1.5 / 3, 1)
    else:
        f = (rn(96, 4), rn(4, 64))
        sd.update({f"{p}qkv.lora_up.weight": f[0], f"{p}qkv.lora_down.weight": f[1], f"{p}qkv.alpha": torch.tensor(2.0)})
        want["qkv"] = ("lora", (f[0], f[1] * 2.0 / 4), 1.0, 1)
    ri = lambda *s: torch.randint(-4, 5, s, generator=g) / 8.0  # small dyadic factors: w2_a @ w2_b is exact in any order, on any device
    w1, w2a, w2b = rn(6, 4), ri(8, 2), ri(2, 16)
    sd.update({f"{p}proj.lokr_w1": w1, f"{p}proj.lokr_w2_a": w2a, f"{p}proj.lokr_w2_b": w2b, f"{p}proj.alpha": torch.tensor(1.0)})
    want["proj"] = ("lokr", (w1, w2a @ w2b), 1.0 / 2, 1)
    return sd, want


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["apply", "load_loras", "load_unload"])
def test_loader_fuses_lycoris_modules(dev, mode):
    """on the parent commit the LoHa / LoKr layers come back unchanged: the loader returned success and did nothing"""
    import lora_loading as ll
    from fluxmi import ops

    model = toy_model(dev)
    state = lambda: {n: (m.float8_data.cpu().view(torch.uint8), m.scale.cpu(), m.scale_reciprocal.cpu()) for n, m in model.double_blocks[0].img_attn.named_children()}
    before = state()
    (sd_a, want_a), (sd_b, want_b) = toy_adapter(1), toy_adapter(2)
    resolve = lambda sd: ll.resolve_lora_state_dict(dict(sd))[1]
    if mode == "apply":
        ll.apply_lora_to_model(model, resolve(sd_a), 0.8)
        steps = [[(want_a, 0.8)]]
    elif mode == "load_loras":
        ll.apply_loras_to_model(model, [(resolve(sd_a), 0.8), (resolve(sd_b), -0.5)])
        steps = [[(want_a, 0.8), (want_b, -0.5)]]
    else:
        ll.apply_lora_to_model(model, resolve(sd_a), 0.8)
        ll.remove_lora_from_module(model, resolve(sd_a), 0.8)
        steps = [[(want_a, 0.8)], [(want_a, -0.8)]]
    after = state()
    for name in ("qkv", "proj"):
        exp = before[name]
        for step in steps:
            terms = [ops.Delta(w[name][0], w[name][1], w[name][2] * s, w[name][3]) for w, s in step]
            exp = restate(exp[0].view(torch.float8_e4m3fn), exp[2], terms, fp64=True)
        assert not torch.equal(after[name][0], before[name][0]), f"{name}: the adapter changed nothing"
        gate(after[name], exp, name == "proj", f"loader {mode} {name}")
