"""fp64 references for the HAT tests, written the way hat_arch.py builds its attention (torch.roll, window_partition, nn.Unfold with zero
padding for the overlapping keys, the gather table[index], the img_mask slices) -- on purpose NOT the addressing of include/fluxmi.h -- and
the whole network (the definition in modules/hat.py's docstring) with a rounding hook at the native path's rounding points."""
import torch
import torch.nn.functional as F

WS, EXT = 16, 24
MEAN = torch.tensor((0.4488, 0.4371, 0.4040), dtype=torch.float64)


def attention16_ref64(q, k, v, table, index, shift, overlap, scale, round=lambda t: t):
    """q, k, v [B, H, W, heads, head_dim], table [rows, heads], index [256, 256 | 576] (torch's indexing: negative entries count from the
    end) -> (out, A) fp64 [B, H, W, heads, head_dim]; A = softmax . |v|.  `round` is applied to the unnormalised probabilities."""
    q, k, v, table = (t.double() for t in (q, k, v, table))
    B, H, W, nh, hd = q.shape

    def windows(t):  # roll, window_partition, heads in front: [B * nW, heads, 256, head_dim]
        t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2)) if shift else t
        t = t.reshape(B, H // WS, WS, W // WS, WS, nh, hd).transpose(2, 3).reshape(-1, WS * WS, nh, hd)
        return t.transpose(1, 2)
    def unfolded(t):  # nn.Unfold(24, stride 16, padding 4) on NCHW, 'b (nc ch owh oww) nw -> (b nw) nc (owh oww) ch'
        u = F.unfold(t.reshape(B, H, W, nh * hd).permute(0, 3, 1, 2), kernel_size=EXT, stride=WS, padding=(EXT - WS) // 2)
        return u.view(B, nh, hd, EXT * EXT, -1).permute(0, 4, 1, 3, 2).reshape(-1, nh, EXT * EXT, hd)
    def reverse(t):  # back to [B, H, W, heads, head_dim], rolled back
        t = t.transpose(1, 2).reshape(B, H // WS, W // WS, WS, WS, nh, hd).transpose(2, 3).reshape(B, H, W, nh, hd)
        return torch.roll(t, shifts=(shift, shift), dims=(1, 2)) if shift else t

    kw, vw = (unfolded(k), unfolded(v)) if overlap else (windows(k), windows(v))
    nk = kw.shape[2]
    bias = table[index.long().view(-1)].view(WS * WS, nk, nh).permute(2, 0, 1)
    attn = (windows(q) * scale) @ kw.transpose(-2, -1) + bias[None]
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
        attn = (attn.view(B, nW, nh, WS * WS, nk) + attn_mask[None, :, None]).view(-1, nh, WS * WS, nk)
    p = torch.exp(attn - attn.amax(-1, keepdim=True))
    l = p.sum(-1, keepdim=True)
    p = round(p)
    return reverse(p @ vw / l), reverse(p @ vw.abs() / l)


def channel_combine_ref64(a, b, y, w1, b1, w2, b2, s):
    """a, b, y [B, H, W, C] -> (a + b + s * y * sigmoid(w2 relu(w1 mean_HW(y) + b1) + b2), the gate [B, C]) in fp64"""
    a, b, y, w1, b1, w2, b2 = (t.double() for t in (a, b, y, w1, b1, w2, b2))
    g = torch.sigmoid(torch.relu(y.mean((1, 2)) @ w1.T + b1) @ w2.T + b2)
    return a + b + s * y * g[:, None, None, :], g


def hat_ref(sd, x, round=lambda t: t):
    """modules/hat.py's forward in fp64 on NHWC x [B, H, W, 3] in [0, 1] -> [B, s H, s W, 3]; `round` where the native path rounds to bf16
    (every launch's output, P inside the attention, the normalised input and the final sum with the mean)"""
    idx_sa, idx_oca = sd["relative_position_index_SA"], sd["relative_position_index_OCA"]
    sd = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    B, H0, W0, _ = x.shape
    C = sd["conv_first.weight"].shape[0]
    conv = lambda n, t: F.conv2d(t.permute(0, 3, 1, 2), sd[n + ".weight"], sd[n + ".bias"], padding=1).permute(0, 2, 3, 1)  # noqa: E731  NHWC
    lin = lambda n, t: t @ sd[n + ".weight"].T + sd[n + ".bias"]  # noqa: E731
    norm = lambda n, t: round(F.layer_norm(t, (C,), sd[n + ".weight"], sd[n + ".bias"], 1e-5))  # noqa: E731
    shuffle = lambda t: F.pixel_shuffle(t.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)  # noqa: E731
    mlp = lambda p, t: round(t + lin(p + "mlp.fc2", round(F.gelu(round(lin(p + "mlp.fc1", norm(p + "norm2", t)))))))  # noqa: E731

    def attention(p, a, n, index, shift, overlap):
        table = sd[p + a + "relative_position_bias_table"]
        nh = table.shape[1]
        qkv = round(lin(p + a + "qkv", n)).view(B, H, W, 3, nh, C // nh)
        o, _ = attention16_ref64(qkv[:, :, :, 0], qkv[:, :, :, 1], qkv[:, :, :, 2], table, index, shift, overlap, (C // nh) ** -0.5, round)
        return lin(p + a + "proj", round(o).reshape(B, H, W, C))

    xn = round(x.double() - MEAN).permute(0, 3, 1, 2)
    xn = F.pad(xn, (0, (-W0) % WS, 0, (-H0) % WS), mode="reflect").permute(0, 2, 3, 1)
    H, W = xn.shape[1:3]
    feat = round(conv("conv_first", xn))
    t = norm("patch_embed.norm", feat)
    i = 0
    while f"layers.{i}.conv.weight" in sd:
        res, j = t, 0
        while f"layers.{i}.residual_group.blocks.{j}.norm1.weight" in sd:
            p = f"layers.{i}.residual_group.blocks.{j}."
            n = norm(p + "norm1", t)
            y = round(conv(p + "conv_block.cab.2", round(F.gelu(round(conv(p + "conv_block.cab.0", n))))))
            w1, w2 = sd[p + "conv_block.cab.3.attention.1.weight"].flatten(1), sd[p + "conv_block.cab.3.attention.3.weight"].flatten(1)
            pa = round(attention(p, "attn.", n, idx_sa, (j % 2) * (WS // 2), 0))
            t = round(channel_combine_ref64(t, pa, y, w1, sd[p + "conv_block.cab.3.attention.1.bias"], w2, sd[p + "conv_block.cab.3.attention.3.bias"], 0.01)[0])
            t = mlp(p, t)
            j += 1
        p = f"layers.{i}.residual_group.overlap_attn."
        t = mlp(p, round(t + attention(p, "", norm(p + "norm1", t), idx_oca, 0, 4)))
        t = round(conv(f"layers.{i}.conv", t) + res)
        i += 1
    t = round(conv("conv_after_body", norm("norm", t)) + feat)
    t = round(F.leaky_relu(conv("conv_before_upsample.0", t), 0.01))
    t = shuffle(round(conv("upsample.0", t)))
    if "upsample.2.weight" in sd:
        t = shuffle(round(conv("upsample.2", t)))
    t = round(conv("conv_last", t))
    s = t.shape[1] // H
    return round(t[:, : s * H0, : s * W0] + MEAN)
