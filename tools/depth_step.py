"""The Depth Anything estimator both ways: modules/depth.DepthAnythingNative on libfluxmi against transformers' DepthAnythingForDepthEstimation
in bf16 through torch on the same GPU.  The Large geometry (hidden 1024, 24 layers, 16 heads, neck 256 / 512 / 1024 / 1024, fusion 256) with
synthetic weights at --res x --res (518: a 37 x 37 grid, 1370 tokens in 1536 rows), ONE process, the two kinds ALTERNATING (--rounds) so that
clock and thermal drift hit both alike.  Timed with hipEvent pairs; peak memory is torch.cuda.max_memory_allocated over one call.
    python tools/depth_step.py [--size large] [--res 518] [--rounds 5] [--layers N]
  model:               both kinds, median / min / max over the rounds, peak memory, the two depths' distance;
  backbone / decoder:  the native path's two halves on their own;
  preprocess_control:  host to host (PIL resize and normalisation, upload, model, fluxmi_depth_to_map, download) for a --photo W x H image.
Prints one JSON line per figure.  For per-stage kernel times:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/depth_step.py --rounds 1 --native-only
    python tools/depth_step.py --summarize DIR"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flux-fp8-api_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np
import torch

# kernel-name fragments -> the stage a launch is counted under
STAGES = [("text_attention_kernel", "attention"), ("gemm", "GEMM (linears, 1x1, implicit 3x3)"), ("row_norm", "LayerNorm"), ("unary_kernel", "GELU / ReLU"),
          ("resize_bilinear", "bilinear resize"), ("conv3x3_dense", "head 3x3 (dense)"), ("depth_head", "head 1x1 + ReLU"), ("patchify", "patch rows"),
          ("im2col_s2", "stride-2 gather"), ("add_kernel", "fusion sum"), ("minmax", "depth min / max"), ("depth_to_map", "depth -> map")]


def summarize(path):
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True) if os.path.isdir(path) else [path]
    if not files:
        sys.exit("no *kernel_trace.csv under " + path)
    t, n = {}, {}
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            stage = next((s for frag, s in STAGES if frag in name), "torch plumbing (copies, permutes, fills)")
            t[stage] = t.get(stage, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
            n[stage] = n.get(stage, 0) + 1
    total = sum(t.values())
    for s, v in sorted(t.items(), key=lambda kv: -kv[1]):
        print(json.dumps(dict(what="kernel time by stage, one profiler trace (warm-up included)", stage=s, launches=n[s], ms=round(v / 1e6, 3), share=round(v / total, 3))))
    print(json.dumps(dict(what="all kernels of the trace", ms=round(total / 1e6, 3))))


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated() - base, out


def stats(what, xs, **kw):
    print(json.dumps(dict(what=what, median_ms=round(statistics.median(xs), 2), min_ms=round(min(xs), 2), max_ms=round(max(xs), 2), n=len(xs), **kw)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="large", choices=["small", "base", "large"])
    ap.add_argument("--res", type=int, default=518)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=0, help="truncate the backbone to this many layers (0 = the size's own)")
    ap.add_argument("--photo", default="1024x768")
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--summarize")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    import depth_ref as dr
    from fluxmi import synth
    from modules.depth import DepthAnythingNative, depth_input_size

    dev = torch.device("cuda:0")
    over = {}
    if a.layers:
        over = dict(num_hidden_layers=a.layers, out_indices=[max(1, a.layers * k // 4) for k in (1, 2, 3, 4)])
    cfg = synth.depth_anything_config(a.size, **over)
    sd = synth.make_depth_anything_state_dict(cfg, seed=0)
    nat = DepthAnythingNative(cfg)
    nat.load_state_dict(sd, strict=True)
    nat = nat.to(device=dev, dtype=torch.bfloat16)
    hf = None
    if not a.native_only:
        hf = dr.hf_model(cfg)
        hf.load_state_dict(sd, strict=True)
        hf = hf.to(device=dev, dtype=torch.bfloat16)
    g = a.res // 14
    pix = dr.pixel_values(1, g, g).to(dev)
    pix_bf = pix.bfloat16()
    bc = cfg["backbone_config"]
    print(json.dumps(dict(what="geometry", size=a.size, hidden=bc["hidden_size"], layers=bc["num_hidden_layers"], grid=[g, g], tokens=g * g + 1,
                          rows=nat.seq_pad(g, g), padded=nat.padded_sizes())), flush=True)
    run_hf = (lambda: hf(pixel_values=pix_bf).predicted_depth) if hf is not None else None
    with torch.inference_mode():
        timed(lambda: nat(pix))  # warm-up: module load, weight layouts, allocator
        if hf is not None:
            timed(run_hf)
        tn, tt, tb, td, mem_n, mem_t, yn, yt = [], [], [], [], 0, 0, None, None
        for _ in range(a.rounds):
            ms, mem_n, yn = timed(lambda: nat(pix))
            tn.append(ms)
            if hf is not None:
                ms, mem_t, yt = timed(run_hf)
                tt.append(ms)
            ms, _, taps = timed(lambda: nat.features(pix))
            tb.append(ms)
            td.append(timed(lambda: nat.decode(taps))[0])
    stats(f"fluxmi Depth Anything {a.size} {a.res}^2", tn, peak_gib=round(mem_n / 2 ** 30, 3))
    stats("  its backbone", tb)
    stats("  its neck + head", td)
    if hf is not None:
        stats(f"transformers bf16 through torch, {a.size} {a.res}^2", tt, peak_gib=round(mem_t / 2 ** 30, 3))
        d = yn.float() - yt.float()
        print(json.dumps(dict(what="the two depths", rel_l2=float(d.norm() / yt.float().norm()), max_abs=float(d.abs().max()),
                              native_min=float(yn.min()), native_max=float(yn.max()))), flush=True)
    # preprocess_control, host to host: what generate(control_preprocess="depth_anything") adds in front of the VAE encode
    w, h = (int(v) for v in a.photo.split("x"))
    photo = np.random.default_rng(0).integers(0, 256, (h, w, 3), dtype=np.uint8)
    th = []
    for _ in range(a.rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = nat.depth_map(photo, (h, w), a.res).cpu()
        th.append((time.perf_counter() - t0) * 1e3)
    stats(f"depth_map host to host, photo {w}x{h} -> estimator input {depth_input_size(w, h, a.res)} -> map {tuple(m.shape)}", th[1:])


if __name__ == "__main__":
    main()
