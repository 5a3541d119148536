"""The ESRGAN upscaler both ways: modules/upscaler.RRDBNet on fluxmi_conv3x3_dense (five in-place launches per dense block, no concatenation)
against the same network through torch.nn.functional.conv2d (bf16, channels_last, torch.cat per layer) on the same GPU.  The 23-block x4
geometry (nf 64, gc 32) with synthetic weights, ONE process, the two kinds ALTERNATING (--rounds) so that clock and thermal drift hit both
alike.  Timed with hipEvent pairs; peak memory is torch.cuda.max_memory_allocated over one call, reset before it.
    python tools/upscaler_step.py [--size 1024] [--big 2048] [--rounds 5] [--blocks 23]
  at --size:  both kinds, median / min / max over the rounds, peak memory, and the two outputs' distance;
  at --big:   the new path only, one call, for its peak memory; 0 skips it.
Prints one JSON line per figure.  For the kernel's own durations by (Cin, Cout):
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/upscaler_step.py --rounds 1 --big 0 --native-only
    python tools/upscaler_step.py --summarize DIR [--blocks 23]"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flux-fp8-api_amd"))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F


def launch_sequence(num_block, nf=64, gc=32):
    """(Cin, Cout, grid) of every launch of one forward, in order; grid: 1 = input size, 2 / 4 = after the first / second upsample"""
    seq = [(16, nf, 1)]
    for _ in range(num_block * 3):
        seq += [(nf + k * gc, gc, 1) for k in range(4)] + [(nf + 4 * gc, nf, 1)]
    return seq + [(nf, nf, 1), (nf, nf, 2), (nf, nf, 4), (nf, nf, 4), (nf, 3, 4)]


def summarize(path, num_block):
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True) if os.path.isdir(path) else [path]
    if not files:
        sys.exit("no *kernel_trace.csv under " + path)
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            if "conv3x3_dense_kernel" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    seq = launch_sequence(num_block)
    if not rows or len(rows) % len(seq):
        sys.exit(f"{len(rows)} conv3x3_dense launches in the trace are no multiple of the {len(seq)} of one {num_block}-block forward")
    t = {}
    for i, (_, d) in enumerate(rows):
        t.setdefault(seq[i % len(seq)], []).append(d)
    total = sum(sum(d) for d in t.values()) / (len(rows) // len(seq))
    for (cin, cout, grid), d in sorted(t.items(), key=lambda kv: -sum(kv[1])):
        per_fwd = sum(d) / (len(rows) // len(seq))
        print(json.dumps(dict(what="conv3x3_dense launches, one profiler trace", cin=cin, cout=cout, grid_scale=grid, launches_per_forward=len(d) // (len(rows) // len(seq)),
                              mean_us=round(sum(d) / len(d) / 1e3, 1), min_us=round(min(d) / 1e3, 1), max_us=round(max(d) / 1e3, 1),
                              ms_per_forward=round(per_fwd / 1e6, 2), share=round(per_fwd / total, 3))))
    print(json.dumps(dict(what="all conv3x3_dense launches of one forward", ms=round(total / 1e6, 2))))


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


class TorchRRDBNet:
    """the same network on the library path: NCHW-shaped bf16 tensors in channels_last memory, F.conv2d + torch.cat"""

    def __init__(self, sd, num_block, dev):
        self.nb = num_block
        self.p = {k: v.to(dev, torch.bfloat16).contiguous(memory_format=torch.channels_last) if v.ndim == 4 else v.to(dev, torch.bfloat16)
                  for k, v in sd.items()}

    def conv(self, x, name):
        return F.conv2d(x, self.p[name + ".weight"], self.p[name + ".bias"], padding=1)

    @torch.inference_mode()
    def __call__(self, x):  # [B, 3, H, W]
        lr = lambda t: F.leaky_relu(t, 0.2)
        feat = self.conv(x, "conv_first")
        h = feat
        for i in range(self.nb):
            x0 = h
            for j in (1, 2, 3):
                parts = [h]
                for k in (1, 2, 3, 4):
                    parts.append(lr(self.conv(torch.cat(parts, 1), f"body.{i}.rdb{j}.conv{k}")))
                h = self.conv(torch.cat(parts, 1), f"body.{i}.rdb{j}.conv5") * 0.2 + h
            h = h * 0.2 + x0
        t = self.conv(h, "conv_body") + feat
        t = lr(self.conv(F.interpolate(t, scale_factor=2, mode="nearest"), "conv_up1"))
        t = lr(self.conv(F.interpolate(t, scale_factor=2, mode="nearest"), "conv_up2"))
        return self.conv(lr(self.conv(t, "conv_hr")), "conv_last")


def stats(what, xs, **kw):
    print(json.dumps(dict(what=what, median_ms=round(statistics.median(xs), 2), min_ms=round(min(xs), 2), max_ms=round(max(xs), 2), n=len(xs), **kw)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--big", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=23)
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--summarize")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, a.blocks)
    from fluxmi import synth
    from modules.upscaler import RRDBNet

    dev = torch.device("cuda:0")
    sd = synth.make_rrdbnet_state_dict(a.blocks, 64, 32, 4, seed=0)
    net = RRDBNet(sd, device=dev)
    ref = None if a.native_only else TorchRRDBNet(sd, a.blocks, dev)
    x = torch.rand(1, a.size, a.size, 3, generator=torch.Generator().manual_seed(1)).bfloat16().to(dev)
    xt = x.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
    flop = 2 * 9 * a.size * a.size * sum(ci * co * g * g for ci, co, g in [(3, 64, 1)] + launch_sequence(a.blocks)[1:])
    print(json.dumps(dict(what="geometry", blocks=a.blocks, size=a.size, tflop=round(flop / 1e12, 2), launches=len(launch_sequence(a.blocks)),
                          estimate_gib=round(net.memory_estimate(1, a.size, a.size) / 2 ** 30, 2))), flush=True)
    timed(lambda: net(x))  # warm-up: module load, allocator
    if ref is not None:
        timed(lambda: ref(xt))  # warm-up: the library's kernel selection
    tn, tt, mem_n, mem_t, yn, yt = [], [], 0, 0, None, None
    for _ in range(a.rounds):
        ms, mem_n, yn = timed(lambda: net(x))
        tn.append(ms)
        if ref is not None:
            ms, mem_t, yt = timed(lambda: ref(xt))
            tt.append(ms)
    stats(f"fluxmi RRDBNet {a.size}^2 -> {4 * a.size}^2", tn, peak_gib=round(mem_n / 2 ** 30, 2), tflops=round(flop / 1e9 / statistics.median(tn), 1))
    if ref is not None:
        stats(f"torch conv2d RRDBNet {a.size}^2 -> {4 * a.size}^2", tt, peak_gib=round(mem_t / 2 ** 30, 2), tflops=round(flop / 1e9 / statistics.median(tt), 1))
        d = (yn.float() - yt.permute(0, 2, 3, 1).float())
        print(json.dumps(dict(what="the two outputs", rel_l2=float(d.norm() / yt.float().norm()), max_abs=float(d.abs().max()))), flush=True)
    del yn, yt
    if a.big:
        xb = torch.rand(1, a.big, a.big, 3, generator=torch.Generator().manual_seed(2)).bfloat16().to(dev)
        ms, mem, _ = timed(lambda: net(xb))
        print(json.dumps(dict(what=f"fluxmi RRDBNet {a.big}^2 -> {4 * a.big}^2, one call", ms=round(ms, 1), peak_gib=round(mem / 2 ** 30, 2),
                              estimate_gib=round(net.memory_estimate(1, a.big, a.big) / 2 ** 30, 2))), flush=True)


if __name__ == "__main__":
    main()
