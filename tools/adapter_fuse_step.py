"""Whole-model adapter fuses on the Flux-dev geometry (every F8Linear of the 19 double + 38 single blocks, modulation included: 11.8 GB of e4m3 weights, each layer
its own buffer): the reference-shaped path (fluxmi_lora_fuse_f8: dequantise, delta, axpy, amax, quantise through an fp32 workspace) beside
fluxmi_adapter_fuse_f8 (csrc/adapter_fuse.hip: two passes over the fp8 bytes, no workspace).
    python tools/adapter_fuse_step.py [--rounds 5] [--out profiles/adapter_fuse.txt]
Timed, alternating in ONE process after a warm-up round, host clock around a synchronise, median / min / max:
  old_lora16    rank-16 LoRA, one fluxmi_lora_fuse_f8 per layer (the baseline)
  new_lora16    the same adapter as one LORA term per layer
  new_loha16    a rank-16 LoHa            new_lokr16    a LoKr with 16 x 16 blocks
  old_3x        three rank-16 LoRAs, three fluxmi_lora_fuse_f8 per layer (three load_lora calls: three re-quantisations)
  new_3in1      the same three as three terms of one call per layer (load_loras: one re-quantisation)
With --dora, alternating with the above (--only REGEX keeps a subset, e.g. for a kernel trace), a rank-16 LoRA with a magnitude vector per layer:
  dora_apply0 / dora_apply1    fluxmi_adapter_fuse_dora_f8 APPLY on axis 0 / 1 (three tile passes)
  dora_remove0 / dora_remove1  REMOVE with the factors the APPLY in front of it returned (two tile passes)
  torch_dora0 / torch_dora1    the same arithmetic in torch on the GPU: dequantise to fp32, delta, norm, rescale, fluxmi_quantize_weight
All at op level on random bytes and factors: file parsing and key conversion are not in the window.  Also the peak device memory each path
adds over the weights and factors (its workspace), and the traffic bound 3 N K bytes (two reads, one write) over the new path's time.
One JSON line per figure, appended to --out when given."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "flux-fp8-api_amd"), os.path.join(ROOT, "tools"), ROOT):
    sys.path.insert(0, p)
import torch

from jpeg_step import alternate

H, MLP = 3072, 12288
# (N, K, how many): qkv, proj, mlp.0, mlp.2 and the modulation of a double block's two streams; linear1, linear2, modulation of a single block
LAYERS = [(3 * H, H, 38), (H, H, 38), (MLP, H, 38), (H, MLP, 38), (6 * H, H, 38), (3 * H + MLP, H, 38), (H, H + MLP, 38), (3 * H, H, 38)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dora", action="store_true", help="add the DoRA kinds")
    ap.add_argument("--only", default=None, help="regex: time only the kinds it matches")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adapter_fuse_step: needs the GPU")
    from fluxmi import ops

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g) * 0.02
    layers, terms = [], {}
    for N, K, count in LAYERS:
        terms[(N, K)] = dict(lora=[ops.Delta("lora", (rn(N, 16), rn(16, K)), 0.5) for _ in range(3)],
                             loha=ops.Delta("loha", (rn(N, 16), rn(16, K), rn(N, 16), rn(16, K)), 0.5), lokr=ops.Delta("lokr", (rn(N // 16, K // 16), rn(16, 16)), 0.5))
        for _ in range(count):
            w = (torch.randint(0, 127, (N, K), device=dev, generator=g, dtype=torch.uint8) | (torch.randint(0, 2, (N, K), device=dev, generator=g, dtype=torch.uint8) << 7))
            layers.append((w.view(torch.float8_e4m3fn), torch.ones((), device=dev), torch.full((), 1e-3, device=dev)))
    total = sum(w.numel() for w, _, _ in layers)

    def old(n):
        for w, s, r in layers:
            for d in terms[tuple(w.shape)]["lora"][:n]:
                ops.lora_fuse_f8(w, s, r, d.factors[0], d.factors[1], d.scale)

    def new(pick):
        for w, s, r in layers:
            ops.adapter_fuse_f8(w, s, r, pick(terms[tuple(w.shape)]))

    fns = {"old_lora16": lambda: old(1), "new_lora16": lambda: new(lambda t: t["lora"][:1]), "new_loha16": lambda: new(lambda t: [t["loha"]]),
           "new_lokr16": lambda: new(lambda t: [t["lokr"]]), "old_3x": lambda: old(3), "new_3in1": lambda: new(lambda t: t["lora"])}
    if a.dora:
        mags = {(N, K): [torch.rand(n, device=dev, generator=g) * 0.05 * K ** 0.5 + 0.1 for n in (N, K)] for N, K, _ in LAYERS}
        factors = {}

        def apply(axis):
            for i, (w, s, r) in enumerate(layers):
                factors[i, axis] = ops.adapter_fuse_dora_f8(w, s, r, terms[tuple(w.shape)]["lora"][:1], mags[tuple(w.shape)][axis], axis, 0.8)

        def remove(axis):
            for i, (w, s, r) in enumerate(layers):
                ops.adapter_unfuse_dora_f8(w, s, r, terms[tuple(w.shape)]["lora"][:1], factors[i, axis], axis)

        def torch_dora(axis, strength=0.8):
            for w, s, r in layers:
                d = terms[tuple(w.shape)]["lora"][0]
                w32, D = ops.dequant(w, r), d.dense()
                b = strength * (mags[tuple(w.shape)][axis] / ((w32 + D).norm(dim=1 - axis) + 2.0 ** -23))
                a, b = ((1 - strength) + b).unsqueeze(1 - axis), b.unsqueeze(1 - axis)
                q, s2, r2 = ops.quantize_weight((a * w32 + b * D).bfloat16())
                w.copy_(q), s.copy_(s2), r.copy_(r2)

        for axis in (0, 1):
            fns.update({f"dora_apply{axis}": lambda axis=axis: apply(axis), f"dora_remove{axis}": lambda axis=axis: remove(axis),
                        f"torch_dora{axis}": lambda axis=axis: torch_dora(axis)})
    if a.only:
        import re

        fns = {k: fn for k, fn in fns.items() if re.search(a.only, k)}
    peak = {}
    for k, fn in fns.items():  # (also the warm-up of every shape)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() - base
    t = alternate(fns, a.rounds)
    ratio = lambda x, y: round(t[x]["median_ms"] / t[y]["median_ms"], 2) if x in t and y in t else None
    line = json.dumps(dict(what="whole-model adapter fuse, Flux-dev geometry", layers=len(layers), weight_bytes=total, **t, peak_extra_bytes=peak,
                           speedup_lora16=ratio("old_lora16", "new_lora16"), speedup_three_adapters=ratio("old_3x", "new_3in1"),
                           new_lora16_bound_3NK_GBps=round(3 * total / t["new_lora16"]["median_ms"] / 1e6, 1) if "new_lora16" in t else None,
                           **{f"dora_{k}{ax}_over_lora16": ratio(f"dora_{k}{ax}", "new_lora16") for k in ("apply", "remove") for ax in (0, 1)},
                           **{f"torch_over_dora_apply{ax}": ratio(f"torch_dora{ax}", f"dora_apply{ax}") for ax in (0, 1)}))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
