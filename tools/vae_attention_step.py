"""The autoencoder's mid-block attention both ways: AutoEncoder.attention = "gemm" (S = Q K^T, fluxmi_softmax_rows, P V: three launches around a
[P, P] bf16 matrix) against "streaming" (fluxmi_vae_attention: one launch).  Real FLUX autoencoder geometry (ch 128, ch_mult [1, 2, 4, 4], mid
width 512), synthetic weights, ONE process, the two kinds ALTERNATING (--rounds) so that clock and thermal drift hit both alike.  Timed with
hipEvent pairs; peak memory is torch.cuda.max_memory_allocated over one call, reset before it.
    python tools/vae_attention_step.py [--size 1024] [--big 2048] [--rounds 5]
  at --size:  the attention alone (the mid block's _attn on a random [1, h, w, 512] activation) and the whole decode, both ways;
  at --big:   decode and encode_moments with "streaming" only ("gemm" cannot hold the matrix there); 0 skips it.
Prints one JSON line per figure: median, min and max over the rounds.  For the kernels' own durations:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/vae_attention_step.py --rounds 2 --big 0 --attention-only
    python tools/vae_attention_step.py --summarize DIR"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flux-fp8-api_amd"))
sys.path.insert(0, ROOT)
import torch

FULL = dict(resolution=256, in_channels=3, ch=128, out_ch=3, ch_mult=[1, 2, 4, 4], num_res_blocks=2, z_channels=16, scale_factor=0.3611,
            shift_factor=0.1159)


def summarize(path):
    """per kernel of one rocprofv3 kernel trace: calls, mean / min / max duration of the launches with the largest grid of that kernel"""
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True) if os.path.isdir(path) else [path]
    if not files:
        sys.exit("no *kernel_trace.csv under " + path)
    t = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            if "vae_attention_kernel" in name or "softmax_rows_kernel" in name or "gemm" in name.lower():
                short = re.sub(r"\(.*", "", name.replace("void ", "").replace("(anonymous namespace)::", ""))[:90]
                key = (short, int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0))
                t.setdefault(key, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    for (name, grid), d in sorted(t.items(), key=lambda kv: -sum(kv[1])):
        print(json.dumps(dict(what="kernel, one profiler trace", kernel=name, grid_x=grid, calls=len(d), mean_us=round(sum(d) / len(d) / 1e3, 1),
                              min_us=round(min(d) / 1e3, 1), max_us=round(max(d) / 1e3, 1))))


def timed(fn):
    """(milliseconds, peak bytes allocated during the call) of one call"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    del out
    return a.elapsed_time(b), torch.cuda.max_memory_allocated() - base


def report(what, kind, size, samples):
    ms = [s[0] for s in samples]
    print(json.dumps(dict(what=what, kind=kind, size=size, rounds=len(ms), median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3),
                          max_ms=round(max(ms), 3), peak_over_inputs_MiB=round(max(s[1] for s in samples) / 2 ** 20, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--big", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--attention-only", action="store_true")
    ap.add_argument("--summarize")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    from modules.autoencoder import AutoEncoder, AutoEncoderParams

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ae = AutoEncoder(AutoEncoderParams(**FULL)).to(device=dev, dtype=torch.bfloat16)
    g = torch.Generator(device=dev).manual_seed(1)
    kinds = ("gemm", "streaming")

    def with_kind(kind, fn):
        ae.attention = kind
        with torch.inference_mode():
            return fn()

    h = args.size // 8
    act = torch.randn(1, h, h, 512, generator=g, device=dev).bfloat16()
    z = torch.randn(1, 16, h, h, generator=g, device=dev)
    runs = [("mid-block attention (norm, projections, attention, proj_out)", lambda: ae._attn(act, ae.decoder.mid.attn_1))]
    if not args.attention_only:
        runs.append(("decode", lambda: ae.decode(z)))
    for what, fn in runs:
        for kind in kinds:  # warm-up: weight caches, allocator, code objects
            with_kind(kind, fn)
        samples = {k: [] for k in kinds}
        for _ in range(args.rounds):
            for kind in kinds:
                samples[kind].append(timed(lambda: with_kind(kind, fn)))
        for kind in kinds:
            report(what, kind, f"{args.size}x{args.size} (P={h * h})", samples[kind])
    if what and not args.attention_only:
        a, b = (with_kind(k, lambda: ae.decode(z)).float() for k in kinds)
        print(json.dumps(dict(what="decode, streaming vs gemm", size=args.size, rel_l2=((a - b).norm() / b.norm()).item())), flush=True)
        del a, b
    if args.big and not args.attention_only:
        hb = args.big // 8
        zb = torch.randn(1, 16, hb, hb, generator=g, device=dev)
        xb = torch.rand(1, 3, args.big, args.big, generator=g, device=dev) * 2 - 1
        for what, fn in (("decode", lambda: ae.decode(zb)), ("encode_moments", lambda: ae.encode_moments(xb))):
            out = with_kind("streaming", fn)
            finite = bool(torch.isfinite(out.float()).all())
            del out
            samples = [timed(lambda: with_kind("streaming", fn)) for _ in range(max(2, args.rounds // 2))]
            report(what, "streaming", f"{args.big}x{args.big} (P={hb * hb}), finite={finite}", samples)


if __name__ == "__main__":
    main()
