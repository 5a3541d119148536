"""HAT both ways: modules/hat.HAT on libfluxmi against the same network in bf16 through torch (roll / partition copies and nn.Unfold around
scaled_dot_product_attention with the additive bias and mask, F.conv2d, F.linear, F.pixel_shuffle) on the same GPU.  HAT-M x4 (embed 180,
6 groups of 6 blocks + one overlapping block, 6 heads) with synthetic weights, B = 1, ONE process, the two kinds ALTERNATING (--rounds) so
that clock and thermal drift hit both alike.  Timed with hipEvent pairs; peak memory is torch.cuda.max_memory_allocated over one call.
    python tools/hat_step.py [--sizes 256,512] [--rounds 5] [--layers 6]
Prints one JSON line per figure.  For the kernels' own times (tracing only, a run of its own):
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/hat_step.py --sizes 256 --rounds 1 --native-only
    python tools/hat_step.py --summarize DIR"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flux-fp8-api_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
import torch.nn.functional as F

import swinir_step as ss

ss.STAGES = [("window_attention16_kernel", "window attention 16 (256 and 576 keys)"), ("channel_partial", "channel mean"), ("channel_mean", "channel mean"),
             ("channel_combine", "squeeze MLP + block sum"), ("channel_norm_kernel", "LayerNorm"), ("gemm", "GEMM (qkv, proj, fc1, fc2)"),
             ("unary_kernel", "GELU"), ("conv3x3_dense", "3x3 convolutions")]


class TorchHAT:
    """modules/hat.py's forward on bf16 CUDA tensors (NCHW convolutions, token rows in between)"""

    def __init__(self, sd, dev):
        self.sd = {k: v.to(dev, torch.bfloat16) for k, v in sd.items() if v.is_floating_point()}
        self.idx = {n: sd["relative_position_index_" + n].to(dev).view(-1) for n in ("SA", "OCA")}
        self.mean = torch.tensor((0.4488, 0.4371, 0.4040), device=dev, dtype=torch.bfloat16).view(1, 3, 1, 1)
        self.masks = {}

    def mask(self, H, W, dev):
        if (H, W) not in self.masks:
            img = torch.zeros(1, H, W, 1, device=dev)
            cnt = 0
            for hs in (slice(0, -16), slice(-16, -8), slice(-8, None)):
                for ws in (slice(0, -16), slice(-16, -8), slice(-8, None)):
                    img[:, hs, ws, :] = cnt
                    cnt += 1
            mw = img.view(1, H // 16, 16, W // 16, 16).transpose(2, 3).reshape(-1, 256)
            m = mw[:, None] - mw[:, :, None]
            self.masks[(H, W)] = m.masked_fill(m != 0, -100.0).bfloat16()
        return self.masks[(H, W)]

    def __call__(self, x):  # NCHW bf16 in [0, 1], H and W multiples of 16
        sd, C = self.sd, self.sd["conv_first.weight"].shape[0]
        conv = lambda n, t, pad=1: F.conv2d(t, sd[n + ".weight"], sd[n + ".bias"], padding=pad)  # noqa: E731
        lin = lambda n, t: F.linear(t, sd[n + ".weight"], sd[n + ".bias"])  # noqa: E731
        norm = lambda n, t: F.layer_norm(t, (C,), sd[n + ".weight"], sd[n + ".bias"], 1e-5)  # noqa: E731
        image = lambda t: t.transpose(1, 2).reshape(B, C, H, W)  # noqa: E731
        mlp = lambda p, t: t + lin(p + "mlp.fc2", F.gelu(lin(p + "mlp.fc1", norm(p + "norm2", t))))  # noqa: E731
        part = lambda t: t.view(B, H // 16, 16, W // 16, 16, -1).transpose(2, 3).reshape(-1, 256, t.shape[-1])  # noqa: E731
        back = lambda t: t.view(B, H // 16, W // 16, 16, 16, C).transpose(2, 3).reshape(B, H, W, C)  # noqa: E731
        B, _, H, W = x.shape
        feat = conv("conv_first", x - self.mean)
        t = norm("patch_embed.norm", feat.flatten(2).transpose(1, 2))
        i = 0
        while f"layers.{i}.conv.weight" in sd:
            res, j = t, 0
            while f"layers.{i}.residual_group.blocks.{j}.norm1.weight" in sd:
                p, shift = f"layers.{i}.residual_group.blocks.{j}.", (j % 2) * 8
                table = sd[p + "attn.relative_position_bias_table"]
                nh = table.shape[1]
                n = norm(p + "norm1", t)
                y = conv(p + "conv_block.cab.2", F.gelu(conv(p + "conv_block.cab.0", image(n))))
                gate = y.mean((2, 3), keepdim=True)
                gate = torch.sigmoid(conv(p + "conv_block.cab.3.attention.3", F.relu(conv(p + "conv_block.cab.3.attention.1", gate, 0)), 0))
                h = n.view(B, H, W, C)
                if shift:
                    h = torch.roll(h, (-shift, -shift), (1, 2))
                q, k, v = lin(p + "attn.qkv", part(h)).view(-1, 256, 3, nh, C // nh).permute(2, 0, 3, 1, 4)
                bias = table[self.idx["SA"]].view(256, 256, nh).permute(2, 0, 1)[None]
                if shift:
                    bias = (bias[None] + self.mask(H, W, x.device)[None, :, None]).expand(B, -1, -1, -1, -1).reshape(-1, nh, 256, 256)
                a = F.scaled_dot_product_attention(q, k, v, attn_mask=bias.expand(q.shape[0], -1, -1, -1))
                a = back(lin(p + "attn.proj", a.transpose(1, 2).reshape(-1, 256, C)))
                if shift:
                    a = torch.roll(a, (shift, shift), (1, 2))
                t = t + a.view(B, H * W, C) + 0.01 * (y * gate).flatten(2).transpose(1, 2)
                t = mlp(p, t)
                j += 1
            p = f"layers.{i}.residual_group.overlap_attn."
            table = sd[p + "relative_position_bias_table"]
            nh = table.shape[1]
            qkv = lin(p + "qkv", norm(p + "norm1", t)).view(B, H, W, 3, C)
            q = part(qkv[:, :, :, 0]).view(-1, 256, nh, C // nh).transpose(1, 2)
            kv = F.unfold(qkv[:, :, :, 1:].reshape(B, H, W, 2 * C).permute(0, 3, 1, 2), kernel_size=24, stride=16, padding=4)
            k, v = kv.view(B, 2, nh, C // nh, 576, -1).permute(1, 0, 5, 2, 4, 3).reshape(2, -1, nh, 576, C // nh)
            bias = table[self.idx["OCA"]].view(256, 576, nh).permute(2, 0, 1)[None]
            a = F.scaled_dot_product_attention(q, k, v, attn_mask=bias.expand(q.shape[0], -1, -1, -1))
            t = t + back(lin(p + "proj", a.transpose(1, 2).reshape(-1, 256, C))).view(B, H * W, C)
            t = mlp(p, t)
            t = conv(f"layers.{i}.conv", image(t)).flatten(2).transpose(1, 2) + res
            i += 1
        t = conv("conv_after_body", image(norm("norm", t))) + feat
        t = F.leaky_relu(conv("conv_before_upsample.0", t), 0.01)
        t = F.pixel_shuffle(conv("upsample.0", t), 2)
        if "upsample.2.weight" in sd:
            t = F.pixel_shuffle(conv("upsample.2", t), 2)
        return conv("conv_last", t) + self.mean


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--summarize")
    a = ap.parse_args()
    if a.summarize:
        return ss.summarize(a.summarize)
    from fluxmi import synth
    from modules.hat import HAT

    dev = torch.device("cuda:0")
    sd = synth.make_hat_state_dict(180, (6,) * a.layers, (6,) * a.layers, scale=4, seed=0)
    sd = {k: (torch.where(v < 0, v + 1521, v) if k.endswith("_OCA") else v) for k, v in sd.items()}  # CUDA gathers take no negative index
    net = HAT(sd, device=dev)
    ref = None if a.native_only else TorchHAT(sd, dev)
    print(json.dumps(dict(what="geometry", embed_dim=180, padded=net.Cp, layers=a.layers, blocks=6, heads=6, mlp=net.Fp, cab=net.Cm, scale=4)), flush=True)
    with torch.inference_mode():
        for size in (int(s) for s in a.sizes.split(",")):
            x = torch.rand(1, size, size, 3, generator=torch.Generator().manual_seed(1)).bfloat16().to(dev)
            xc = x.permute(0, 3, 1, 2).contiguous()
            ss.timed(lambda: net(x))  # warm-up: code objects, allocator
            if ref is not None:
                ss.timed(lambda: ref(xc))
            tn, tt, mem_n, mem_t, yn, yt = [], [], 0, 0, None, None
            for _ in range(a.rounds):
                ms, mem_n, yn = ss.timed(lambda: net(x))
                tn.append(ms)
                if ref is not None:
                    ms, mem_t, yt = ss.timed(lambda: ref(xc))
                    tt.append(ms)
            ss.stats(f"fluxmi HAT-M x4 {size}^2 -> {4 * size}^2", tn, peak_gib=round(mem_n / 2 ** 30, 3))
            if ref is not None:
                ss.stats(f"torch bf16 (SDPA) HAT-M x4 {size}^2 -> {4 * size}^2", tt, peak_gib=round(mem_t / 2 ** 30, 3))
                d = yn.float() - yt.permute(0, 2, 3, 1).float()
                print(json.dumps(dict(what="the two outputs", size=size, rel_l2=float(d.norm() / yt.float().norm()), max_abs=float(d.abs().max()))), flush=True)
            del yn, yt
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
