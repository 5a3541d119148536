"""SwinIR both ways: modules/swinir.SwinIR on libfluxmi against the same network in bf16 through torch (roll / partition copies around
scaled_dot_product_attention with the additive bias and mask, F.conv2d, F.linear) on the same GPU.  SwinIR-M x4 (embed 180, 6 x 6 blocks,
6 heads, 1conv) with synthetic weights, B = 1, ONE process, the two kinds ALTERNATING (--rounds) so that clock and thermal drift hit both
alike.  Timed with hipEvent pairs; peak memory is torch.cuda.max_memory_allocated over one call.
    python tools/swinir_step.py [--sizes 256,512] [--rounds 5] [--layers 6]
Prints one JSON line per figure.  For the kernels' own times (tracing only, a run of its own):
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/swinir_step.py --sizes 256 --rounds 1 --native-only
    python tools/swinir_step.py --summarize DIR"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flux-fp8-api_amd"))
import torch
import torch.nn.functional as F

STAGES = [("window_attention_kernel", "window attention"), ("channel_norm_kernel", "LayerNorm"), ("gemm", "GEMM (qkv, proj, fc1, fc2)"),
          ("unary_kernel", "GELU"), ("conv3x3_dense", "3x3 convolutions")]


def summarize(path):
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True) if os.path.isdir(path) else [path]
    if not files:
        sys.exit("no *kernel_trace.csv under " + path)
    t, n = {}, {}
    for f in files:
        for r in csv.DictReader(open(f)):
            stage = next((s for frag, s in STAGES if frag in r["Kernel_Name"]), "torch plumbing (copies, fills, pad)")
            t[stage] = t.get(stage, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
            n[stage] = n.get(stage, 0) + 1
    total = sum(t.values())
    for s, v in sorted(t.items(), key=lambda kv: -kv[1]):
        print(json.dumps(dict(what="kernel time by stage, one profiler trace (warm-up included)", stage=s, launches=n[s], ms=round(v / 1e6, 3),
                              us_per_launch=round(v / 1e3 / n[s], 2), share=round(v / total, 3))))
    print(json.dumps(dict(what="all kernels of the trace", ms=round(total / 1e6, 3))))


class TorchSwinIR:
    """KAIR's forward on bf16 CUDA tensors (NCHW convolutions, token rows in between)"""

    def __init__(self, sd, dev):
        self.sd = {k: v.to(dev, torch.bfloat16) for k, v in sd.items() if v.is_floating_point()}
        self.index = next(v for k, v in sd.items() if k.endswith("relative_position_index")).to(dev).view(-1)
        self.mean = torch.tensor((0.4488, 0.4371, 0.4040), device=dev, dtype=torch.bfloat16).view(1, 3, 1, 1)
        self.masks = {}

    def mask(self, H, W, dev):
        if (H, W) not in self.masks:
            img = torch.zeros(1, H, W, 1, device=dev)
            cnt = 0
            for hs in (slice(0, -8), slice(-8, -4), slice(-4, None)):
                for ws in (slice(0, -8), slice(-8, -4), slice(-4, None)):
                    img[:, hs, ws, :] = cnt
                    cnt += 1
            mw = img.view(1, H // 8, 8, W // 8, 8).transpose(2, 3).reshape(-1, 64)
            m = mw[:, None] - mw[:, :, None]
            self.masks[(H, W)] = m.masked_fill(m != 0, -100.0).bfloat16()
        return self.masks[(H, W)]

    def __call__(self, x):  # NCHW bf16 in [0, 1], H and W multiples of 8
        sd, C = self.sd, self.sd["conv_first.weight"].shape[0]
        conv = lambda n, t: F.conv2d(t, sd[n + ".weight"], sd[n + ".bias"], padding=1)  # noqa: E731
        lin = lambda n, t: F.linear(t, sd[n + ".weight"], sd[n + ".bias"])  # noqa: E731
        norm = lambda n, t: F.layer_norm(t, (C,), sd[n + ".weight"], sd[n + ".bias"], 1e-5)  # noqa: E731
        B, _, H, W = x.shape
        feat = conv("conv_first", x - self.mean)
        t = norm("patch_embed.norm", feat.flatten(2).transpose(1, 2))
        i = 0
        while f"layers.{i}.conv.weight" in sd:
            res, j = t, 0
            while f"layers.{i}.residual_group.blocks.{j}.norm1.weight" in sd:
                p, shift = f"layers.{i}.residual_group.blocks.{j}.", (j % 2) * 4
                table = sd[p + "attn.relative_position_bias_table"]
                nh = table.shape[1]
                h = norm(p + "norm1", t).view(B, H, W, C)
                if shift:
                    h = torch.roll(h, (-shift, -shift), (1, 2))
                h = h.view(B, H // 8, 8, W // 8, 8, C).transpose(2, 3).reshape(-1, 64, C)
                q, k, v = lin(p + "attn.qkv", h).view(-1, 64, 3, nh, C // nh).permute(2, 0, 3, 1, 4)
                bias = table[self.index].view(64, 64, nh).permute(2, 0, 1)[None]
                if shift:
                    bias = (bias[None] + self.mask(H, W, x.device)[None, :, None]).expand(B, -1, -1, -1, -1).reshape(-1, nh, 64, 64)
                a = F.scaled_dot_product_attention(q, k, v, attn_mask=bias.expand(q.shape[0], -1, -1, -1))
                a = lin(p + "attn.proj", a.transpose(1, 2).reshape(-1, 64, C))
                a = a.view(B, H // 8, W // 8, 8, 8, C).transpose(2, 3).reshape(B, H, W, C)
                if shift:
                    a = torch.roll(a, (shift, shift), (1, 2))
                t = t + a.view(B, H * W, C)
                t = t + lin(p + "mlp.fc2", F.gelu(lin(p + "mlp.fc1", norm(p + "norm2", t))))
                j += 1
            t = conv(f"layers.{i}.conv", t.transpose(1, 2).reshape(B, C, H, W)).flatten(2).transpose(1, 2) + res
            i += 1
        t = conv("conv_after_body", norm("norm", t).transpose(1, 2).reshape(B, C, H, W)) + feat
        t = F.leaky_relu(conv("conv_before_upsample.0", t), 0.01)
        t = F.leaky_relu(conv("conv_up1", F.interpolate(t, scale_factor=2, mode="nearest")), 0.2)
        t = F.leaky_relu(conv("conv_up2", F.interpolate(t, scale_factor=2, mode="nearest")), 0.2)
        return conv("conv_last", F.leaky_relu(conv("conv_hr", t), 0.2)) + self.mean


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
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--summarize")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    from fluxmi import synth
    from modules.swinir import SwinIR

    dev = torch.device("cuda:0")
    sd = synth.make_swinir_state_dict(180, (6,) * a.layers, (6,) * a.layers, 2.0, "1conv", 4, seed=0)
    net = SwinIR(sd, device=dev)
    ref = None if a.native_only else TorchSwinIR(sd, dev)
    print(json.dumps(dict(what="geometry", embed_dim=180, padded=net.Cp, layers=a.layers, blocks=6, heads=6, mlp=net.Fp, scale=4)), flush=True)
    with torch.inference_mode():
        for size in (int(s) for s in a.sizes.split(",")):
            x = torch.rand(1, size, size, 3, generator=torch.Generator().manual_seed(1)).bfloat16().to(dev)
            xc = x.permute(0, 3, 1, 2).contiguous()
            timed(lambda: net(x))  # warm-up: code objects, allocator
            if ref is not None:
                timed(lambda: ref(xc))
            tn, tt, mem_n, mem_t, yn, yt = [], [], 0, 0, None, None
            for _ in range(a.rounds):
                ms, mem_n, yn = timed(lambda: net(x))
                tn.append(ms)
                if ref is not None:
                    ms, mem_t, yt = timed(lambda: ref(xc))
                    tt.append(ms)
            stats(f"fluxmi SwinIR-M x4 {size}^2 -> {4 * size}^2", tn, peak_gib=round(mem_n / 2 ** 30, 3))
            if ref is not None:
                stats(f"torch bf16 (SDPA) SwinIR-M x4 {size}^2 -> {4 * size}^2", tt, peak_gib=round(mem_t / 2 ** 30, 3))
                d = yn.float() - yt.permute(0, 2, 3, 1).float()
                print(json.dumps(dict(what="the two outputs", size=size, rel_l2=float(d.norm() / yt.float().norm()), max_abs=float(d.abs().max()))), flush=True)
            del yn, yt
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
