"""References of the Depth Anything depth estimator (modules/depth.py, csrc/depth.hip), shared by tests/test_depth_cpu.py and
tests/test_depth_gpu.py.

`forward` restates the arithmetic of transformers' DepthAnythingForDepthEstimation (a DINOv2 backbone, the DPT reassemble / fusion neck,
the three-convolution head) in plain torch, in fp64, from a state dict in transformers' key layout; every size is read from the tensors, so
the channel-padded state dict of DepthAnythingNative.padded_state_dict() runs through it unchanged.  `dtype`:
  torch.float64   no rounding anywhere: equals the transformers model in double up to summation order (tests/test_depth_cpu.py)
  torch.bfloat16  the same fp64 arithmetic with a bf16 rounding at every point where the native path stores a bf16 tensor (weights, the
                  pixel values, every GEMM / convolution output, the gate * y and the residual sum of the gate-residual epilogue,
                  LayerNorm, GELU, P of the attention and its output before and after the V bias, every resize); the head's last 1x1
                  convolution + ReLU stays unrounded, as fluxmi_depth_head keeps it in fp32.  Its distance to the fp64 run is the yardstick
                  the native model is held to.  Resize coordinates are then fp32, as the kernel (and torch on fp32 / bf16) computes them.
The position embedding is interpolated in fp32 whatever the dtype: Dinov2Embeddings.interpolate_pos_encoding casts to fp32 itself.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from parity_util import round_fp64_to_bf16

GRIDS = [(1, 1), (3, 5), (4, 4), (2, 7)]
# depth -> map: ((h, w) of the depth, (H, W) of the map): one source pixel, up, down, mixed, the identity, a row wider than one workgroup's 1024 pixels
MAP_CASES = [((1, 1), (5, 7)), ((14, 14), (64, 61)), ((42, 70), (96, 64)), ((56, 56), (30, 31)), ((28, 98), (28, 98)), ((14, 70), (3, 1030))]
PATCH = 14
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def tiny_config(**over) -> dict:
    """config.json of the tiny geometry: hidden 128, 2 heads of 64, 4 layers tapped at 1..4, neck [64, 128, 128, 128], fusion 64, head 32, a
    37 x 37 position grid (so that every grid of GRIDS interpolates)"""
    bc = dict(model_type="dinov2", hidden_size=128, num_attention_heads=2, num_hidden_layers=4, image_size=518, patch_size=PATCH,
              out_indices=[1, 2, 3, 4], apply_layernorm=True, reshape_hidden_states=False, layerscale_value=1.0, mlp_ratio=4)
    c = dict(model_type="depth_anything", backbone_config=bc, reassemble_hidden_size=128, neck_hidden_sizes=[64, 128, 128, 128],
             fusion_hidden_size=64, head_hidden_size=32, reassemble_factors=[4, 2, 1, 0.5], patch_size=PATCH)
    for k, v in over.items():
        if k in bc or k in ("use_swiglu_ffn", "hidden_act", "qkv_bias", "layer_norm_eps", "out_features", "num_channels"):
            bc[k] = v
        else:
            c[k] = v
    return c


def hf_model(cfg: dict):
    """transformers' model of a config dict, random weights, eval mode"""
    from transformers import DepthAnythingConfig, DepthAnythingForDepthEstimation, Dinov2Config

    bc = {k: v for k, v in cfg["backbone_config"].items() if k != "model_type"}
    c = DepthAnythingConfig(backbone_config=Dinov2Config(**bc), **{k: v for k, v in cfg.items() if k not in ("backbone_config", "model_type")})
    return DepthAnythingForDepthEstimation(c).eval()


def pixel_values(B, gh, gw, seed=0):
    """fp32 [B, 3, 14 gh, 14 gw]: smooth ramps + noise, normalised like a photo (values around -2 .. 2.5)"""
    g = torch.Generator().manual_seed(1000 * seed + 31 * gh + gw)
    H, W = PATCH * gh, PATCH * gw
    yy, xx = torch.linspace(0, 1, H)[:, None], torch.linspace(0, 1, W)[None, :]
    out = []
    for b in range(B):
        ph = torch.rand(3, 2, generator=g)
        img = torch.stack([0.5 + 0.4 * torch.sin(6.0 * (yy * ph[c, 0] + xx * ph[c, 1]) + b) for c in range(3)])
        img = (img + 0.1 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
        out.append(torch.stack([(img[c] - IMAGENET_MEAN[c]) / IMAGENET_STD[c] for c in range(3)]))
    return torch.stack(out).float()


# ---- pieces ---------------------------------------------------------------------------------------------------------------------------------
def _rounder(dtype):
    if dtype == torch.float64:
        return lambda x: x
    assert dtype == torch.bfloat16, dtype
    return lambda x: round_fp64_to_bf16(x).double()


def interpolate_pos(pos: torch.Tensor, gh: int, gw: int) -> torch.Tensor:
    """Dinov2Embeddings.interpolate_pos_encoding: pos [1, 1 + n^2, D] -> [1 + gh gw, D] in pos's dtype; the patch rows go to fp32, through
    a bicubic align_corners=False resize and back, the class row is untouched; the stored table itself when the grid is the checkpoint's"""
    n = pos.shape[1] - 1
    s = int(n ** 0.5)
    if gh * gw == n and gh == gw:
        return pos[0]
    D = pos.shape[-1]
    grid = pos[:, 1:].reshape(1, s, s, D).permute(0, 3, 1, 2).float()
    grid = F.interpolate(grid, size=(gh, gw), mode="bicubic", align_corners=False).to(pos.dtype)
    return torch.cat((pos[0, :1], grid.permute(0, 2, 3, 1).reshape(gh * gw, D)), 0)


def ac_coords(n_in: int, n_out: int, fp32: bool):
    """align_corners=True source of every output index: (i0, i1, l1) with l1 in fp64; fp32=True computes scale and scale * o in fp32 as the
    kernel and torch's fp32 path do, else in fp64"""
    o = np.arange(n_out)
    if fp32:
        scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
        src = (scale * o.astype(np.float32)).astype(np.float32)
    else:
        src = ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0) * o.astype(np.float64)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy((src.astype(np.float64) - i0))


def resize_ac(x: torch.Tensor, Ho: int, Wo: int, fp32_coords: bool) -> torch.Tensor:
    """x fp64 [..., Hi, Wi] -> [..., Ho, Wo], bilinear with align_corners=True"""
    Hi, Wi = x.shape[-2:]
    y0, y1, ly = ac_coords(Hi, Ho, fp32_coords)
    x0, x1, lx = ac_coords(Wi, Wo, fp32_coords)
    ly, lx = ly[:, None], lx[None, :]
    top = (1 - lx) * x[..., y0, :][..., :, x0] + lx * x[..., y0, :][..., :, x1]
    bot = (1 - lx) * x[..., y1, :][..., :, x0] + lx * x[..., y1, :][..., :, x1]
    return (1 - ly) * top + ly * bot


def resize_taps_abs(x: torch.Tensor, Ho: int, Wo: int) -> torch.Tensor:
    """sum of the four |weight x tap| of resize_ac(x, fp32 coordinates): the magnitude the fp32 blend's rounding errors scale with"""
    return resize_ac(x.abs(), Ho, Wo, True)


def gelu_erf(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _ln(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def backbone(sd, cfg, pix, dtype=torch.float64):
    """-> the tapped hidden states, each fp64 [B, gh gw, D] (final LayerNorm applied when the config says so, class row dropped)"""
    r = _rounder(dtype)
    W = lambda k: r(sd[k].double())  # noqa: E731
    bc = cfg["backbone_config"]
    D, H, eps = bc["hidden_size"], bc["num_attention_heads"], bc.get("layer_norm_eps", 1e-6)
    B, _, Hp, Wp = pix.shape
    gh, gw = Hp // PATCH, Wp // PATCH
    e = "backbone.embeddings."
    x = r(F.conv2d(r(pix.double()), W(e + "patch_embeddings.projection.weight"), W(e + "patch_embeddings.projection.bias"), stride=PATCH))
    x = x.flatten(2).transpose(1, 2)  # [B, gh gw, D]
    pos = r(interpolate_pos(sd[e + "position_embeddings"] if dtype == torch.float64 else r(sd[e + "position_embeddings"].double()), gh, gw).double())
    x = torch.cat((r(W(e + "cls_token")[0] + pos[:1]).expand(B, 1, D), r(x + pos[1:])), 1)
    hd = D // H
    taps = []
    n_layers = bc["num_hidden_layers"]
    want = out_indices(cfg)
    for i in range(n_layers):
        p = f"backbone.encoder.layer.{i}."
        h = r(_ln(x, W(p + "norm1.weight"), W(p + "norm1.bias"), eps))
        q, k, v = (r(h @ W(p + f"attention.attention.{n}.weight").T + (W(p + f"attention.attention.{n}.bias") if n != "value" else 0))
                   for n in ("query", "key", "value"))
        split = lambda t: t.view(B, -1, H, hd).transpose(1, 2)  # noqa: E731
        pr = r(torch.softmax(split(q) @ split(k).transpose(-1, -2) * hd ** -0.5, -1))
        o = r(r((pr @ split(v)).transpose(1, 2).reshape(B, -1, D)) + W(p + "attention.attention.value.bias"))
        a = r(o @ W(p + "attention.output.dense.weight").T + W(p + "attention.output.dense.bias"))
        x = r(x + r(W(p + "layer_scale1.lambda1") * a))
        h = r(_ln(x, W(p + "norm2.weight"), W(p + "norm2.bias"), eps))
        f = r(gelu_erf(r(h @ W(p + "mlp.fc1.weight").T + W(p + "mlp.fc1.bias"))))
        m = r(f @ W(p + "mlp.fc2.weight").T + W(p + "mlp.fc2.bias"))
        x = r(x + r(W(p + "layer_scale2.lambda1") * m))
        if i + 1 in want:
            y = r(_ln(x, W("backbone.layernorm.weight"), W("backbone.layernorm.bias"), eps)) if bc.get("apply_layernorm", True) else x
            taps.append(y[:, 1:])
    return taps


def out_indices(cfg) -> list:
    bc = cfg["backbone_config"]
    if bc.get("out_indices") is not None:
        return [int(i) for i in bc["out_indices"]]
    if bc.get("out_features") is not None:
        return [int(s[len("stage"):]) for s in bc["out_features"]]
    return [bc["num_hidden_layers"]]


def decoder(sd, cfg, taps, gh, gw, dtype=torch.float64):
    """the neck and the head on the tapped hidden states -> predicted_depth fp64 [B, 14 gh, 14 gw]"""
    r = _rounder(dtype)
    W = lambda k: r(sd[k].double())  # noqa: E731
    c32 = dtype != torch.float64
    conv = lambda x, k, **kw: r(F.conv2d(x, W(k + ".weight"), W(k + ".bias") if k + ".bias" in sd else None, **kw))  # noqa: E731
    feats = []
    for i, (t, f) in enumerate(zip(taps, cfg.get("reassemble_factors", [4, 2, 1, 0.5]))):
        B = t.shape[0]
        x = t.reshape(B, gh, gw, -1).permute(0, 3, 1, 2)
        p = f"neck.reassemble_stage.layers.{i}."
        x = conv(x, p + "projection")
        if f > 1:
            x = r(F.conv_transpose2d(x, W(p + "resize.weight"), W(p + "resize.bias"), stride=int(f)))
        elif f < 1:
            x = conv(x, p + "resize", stride=int(round(1 / f)), padding=1)
        feats.append(conv(x, f"neck.convs.{i}", padding=1))

    def rcu(x, p):
        h = conv(torch.relu(x), p + "convolution1", padding=1)
        h = conv(torch.relu(h), p + "convolution2", padding=1)
        return r(x + h)

    feats = feats[::-1]
    fused = None
    for k, f in enumerate(feats):
        p = f"neck.fusion_stage.layers.{k}."
        fused = f if fused is None else r(fused + rcu(f, p + "residual_layer1."))
        fused = rcu(fused, p + "residual_layer2.")
        size = feats[k + 1].shape[-2:] if k + 1 < len(feats) else (2 * fused.shape[-2], 2 * fused.shape[-1])
        fused = conv(r(resize_ac(fused, size[0], size[1], c32)), p + "projection")
    x = conv(fused, "head.conv1", padding=1)
    x = r(resize_ac(x, PATCH * gh, PATCH * gw, c32))
    x = r(torch.relu(F.conv2d(x, W("head.conv2.weight"), W("head.conv2.bias"), padding=1)))
    x = torch.relu(F.conv2d(x, W("head.conv3.weight"), W("head.conv3.bias")))
    return x[:, 0] * cfg.get("max_depth", 1)


def forward(sd, cfg, pix, dtype=torch.float64):
    """pixel_values [B, 3, 14 gh, 14 gw] -> predicted_depth fp64 [B, 14 gh, 14 gw]"""
    gh, gw = pix.shape[-2] // PATCH, pix.shape[-1] // PATCH
    with torch.no_grad():
        return decoder(sd, cfg, backbone(sd, cfg, pix, dtype), gh, gw, dtype)


def rel_l2(a, b) -> float:
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---- depth -> control map -----------------------------------------------------------------------------------------------------------------
def hp_coords(n_in: int, n_out: int):
    """half-pixel (align_corners=False) source of every output index, scale and source in fp32 as include/fluxmi.h states -> (i0, i1, l1 fp64)"""
    scale = np.float32(n_in) / np.float32(n_out)
    src = (scale * (np.arange(n_out).astype(np.float32) + np.float32(0.5))).astype(np.float32) - np.float32(0.5)
    src = np.maximum(src.astype(np.float32), np.float32(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, np.minimum(src.astype(np.float64) - i0, 1.0)


def depth_to_map_f64(depth: np.ndarray, H: int, W: int, normalize: str = "minmax") -> np.ndarray:
    """depth [B, h, w] -> the fp64 value t of include/fluxmi.h (before floor(t + 0.5) and the clamp), [B, H, W]"""
    d = depth.astype(np.float64)
    B, h, w = d.shape
    y0, y1, ly = hp_coords(h, H)
    x0, x1, lx = hp_coords(w, W)
    ly, lx = ly[None, :, None], lx[None, None, :]
    top = (1 - lx) * d[:, y0][:, :, x0] + lx * d[:, y0][:, :, x1]
    bot = (1 - lx) * d[:, y1][:, :, x0] + lx * d[:, y1][:, :, x1]
    v = (1 - ly) * top + ly * bot
    if normalize == "raw":
        return v
    mn, mx = d.reshape(B, -1).min(1)[:, None, None], d.reshape(B, -1).max(1)[:, None, None]
    rng = np.where(mx > mn, mx - mn, 1.0)
    return np.where(mx > mn, (v - mn) * (255.0 / rng), 0.0)


def map_bytes(t: np.ndarray) -> np.ndarray:
    return np.clip(np.floor(t + 0.5), 0, 255).astype(np.uint8)


def map_excused(t: np.ndarray) -> np.ndarray:
    """pixels whose fp64 value lies within 2^-10 of a half-integer (where floor(t + 0.5) steps): an fp32 blend may land on either side"""
    f = t + 0.5
    return np.abs(f - np.rint(f)) < 2.0 ** -10


def depth_samples(B, h, w, seed=0) -> np.ndarray:
    """positive fp32 depths with structure: a ramp + blobs + a little noise, different per image"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for b in range(B):
        d = 0.3 + 0.05 * b + 2.0 * yy / max(h - 1, 1) + 0.7 * np.sin(0.37 * xx + b) * np.cos(0.23 * yy) + 0.05 * rng.standard_normal((h, w))
        out.append(np.abs(d) * (3.0 + b))
    return np.stack(out).astype(np.float32)
