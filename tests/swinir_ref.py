"""fp64 references for the SwinIR tests: the shifted-window attention written the way KAIR's network_swinir.py writes it (torch.roll,
window_partition, the relative_position_index table, the img_mask slices) -- on purpose NOT the closed form of include/fluxmi.h -- and the
whole network with a rounding hook at the native path's rounding points (modules/swinir.py)."""
import torch
import torch.nn.functional as F

WS = 8
MEAN = torch.tensor((0.4488, 0.4371, 0.4040), dtype=torch.float64)


def window_attention_ref64(q, k, v, table, shift, scale, round=lambda t: t):
    """q, k, v [B, H, W, heads, head_dim], table [225, heads] -> (out, A) fp64 [B, H, W, heads, head_dim]; A = softmax . |v|.
    `round` is applied to the unnormalised probabilities exp(t - max), where the kernel rounds P to bf16."""
    q, k, v, table = (t.double() for t in (q, k, v, table))
    B, H, W, nh, hd = q.shape

    def partition(t):  # [B, H, W, ...] -> [B * nW, 64, ...]
        t = t.reshape(B, H // WS, WS, W // WS, WS, *t.shape[3:])
        return t.transpose(2, 3).reshape(-1, WS * WS, *t.shape[5:])
    def windows(t):  # roll, partition, heads in front: [B * nW, heads, 64, head_dim]
        t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2)) if shift else t
        return partition(t).transpose(1, 2)
    def reverse(t):  # back to [B, H, W, heads, head_dim], rolled back
        t = t.transpose(1, 2).reshape(B, H // WS, W // WS, WS, WS, nh, hd).transpose(2, 3).reshape(B, H, W, nh, hd)
        return torch.roll(t, shifts=(shift, shift), dims=(1, 2)) if shift else t

    coords = torch.stack(torch.meshgrid(torch.arange(WS), torch.arange(WS), indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += WS - 1
    rel[:, :, 1] += WS - 1
    rel[:, :, 0] *= 2 * WS - 1
    index = rel.sum(-1)
    bias = table[index.view(-1)].view(WS * WS, WS * WS, nh).permute(2, 0, 1)
    attn = (windows(q) * scale) @ windows(k).transpose(-2, -1) + bias[None]
    if shift:
        img_mask = torch.zeros(1, H, W, 1, dtype=torch.float64)
        cnt = 0
        for hs in (slice(0, -WS), slice(-WS, -shift), slice(-shift, None)):
            for ws in (slice(0, -WS), slice(-WS, -shift), slice(-shift, None)):
                img_mask[:, hs, ws, :] = cnt
                cnt += 1
        mw = img_mask.reshape(1, H // WS, WS, W // WS, WS).transpose(2, 3).reshape(-1, WS * WS)
        attn_mask = mw[:, None] - mw[:, :, None]
        attn_mask = attn_mask.masked_fill(attn_mask != 0, -100.0)
        nW = attn_mask.shape[0]
        attn = (attn.view(B, nW, nh, WS * WS, WS * WS) + attn_mask[None, :, None]).view(-1, nh, WS * WS, WS * WS)
    p = torch.exp(attn - attn.amax(-1, keepdim=True))
    l = p.sum(-1, keepdim=True)
    p = round(p)
    vw = windows(v)
    return reverse(p @ vw / l), reverse(p @ vw.abs() / l)


def swinir_ref(sd, x, round=lambda t: t):
    """KAIR's SwinIR forward ("nearest+conv") in fp64 on NHWC x [B, H, W, 3] in [0, 1] -> [B, s H, s W, 3]; `round` where the native path
    rounds to bf16 (every launch's output, P inside the attention, the normalised input and the final sum with the mean)"""
    sd = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    B, H0, W0, _ = x.shape
    C = sd["conv_first.weight"].shape[0]
    conv = lambda n, t, pad=1: F.conv2d(t.permute(0, 3, 1, 2), sd[n + ".weight"], sd[n + ".bias"], padding=pad).permute(0, 2, 3, 1)  # noqa: E731  NHWC
    lin = lambda n, t: t @ sd[n + ".weight"].T + sd[n + ".bias"]  # noqa: E731
    norm = lambda n, t: round(F.layer_norm(t, (C,), sd[n + ".weight"], sd[n + ".bias"], 1e-5))  # noqa: E731
    up2 = lambda t: t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)  # noqa: E731

    def body_conv(name, t, res):
        if name + ".weight" in sd:
            return round(conv(name, t) + res)
        t = round(F.leaky_relu(conv(name + ".0", t), 0.2))
        t = round(F.leaky_relu(conv(name + ".2", t, pad=0), 0.2))
        return round(conv(name + ".4", t) + res)

    xn = round(x.double() - MEAN).permute(0, 3, 1, 2)
    xn = F.pad(xn, (0, (-W0) % WS, 0, (-H0) % WS), mode="reflect").permute(0, 2, 3, 1)
    H, W = xn.shape[1:3]
    feat = round(conv("conv_first", xn))
    t = norm("patch_embed.norm", feat)
    i = 0
    while f"layers.{i}.residual_group.blocks.0.norm1.weight" in sd:
        res, j = t, 0
        while f"layers.{i}.residual_group.blocks.{j}.norm1.weight" in sd:
            p = f"layers.{i}.residual_group.blocks.{j}."
            table = sd[p + "attn.relative_position_bias_table"]
            nh = table.shape[1]
            qkv = round(lin(p + "attn.qkv", norm(p + "norm1", t))).view(B, H, W, 3, nh, C // nh)
            a, _ = window_attention_ref64(qkv[:, :, :, 0], qkv[:, :, :, 1], qkv[:, :, :, 2], table, (j % 2) * (WS // 2), (C // nh) ** -0.5, round)
            t = round(t + lin(p + "attn.proj", round(a).reshape(B, H, W, C)))
            f = round(F.gelu(round(lin(p + "mlp.fc1", norm(p + "norm2", t)))))
            t = round(t + lin(p + "mlp.fc2", f))
            j += 1
        t = body_conv(f"layers.{i}.conv", t, res)
        i += 1
    t = body_conv("conv_after_body", norm("norm", t), feat)
    t = round(F.leaky_relu(conv("conv_before_upsample.0", t), 0.01))
    t = round(F.leaky_relu(conv("conv_up1", up2(t)), 0.2))
    if "conv_up2.weight" in sd:
        t = round(F.leaky_relu(conv("conv_up2", up2(t)), 0.2))
    t = round(conv("conv_last", round(F.leaky_relu(conv("conv_hr", t), 0.2))))
    s = t.shape[1] // H
    return round(t[:, : s * H0, : s * W0] + MEAN)
