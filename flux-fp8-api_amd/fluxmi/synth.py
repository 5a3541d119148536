"""Synthetic Flux checkpoints and inputs (no real weights exist offline).

Produces a BFL-format state dict (key names / shapes of SURVEY.md Appendix D, i.e. what
`util.load_flow_model` feeds to `Flux.load_state_dict`) from a seed, plus the seeded synthetic
request tensors of SURVEY.md §8(d).  Pure torch, CPU by default so that the bytes are identical on
every machine; pass device="cuda" for the full 12 B-parameter bench model (device RNG, not portable,
parity tests never use it).
"""
from __future__ import annotations

import math
from typing import Dict

import torch


def _linear(sd, name, n_out, n_in, gen, device, dtype, gain=1.0, bias=True, outliers=True):
    bound = gain * math.sqrt(3.0 / n_in)
    w = (torch.rand(n_out, n_in, generator=gen, device=device, dtype=torch.float32) * 2 - 1) * bound
    if outliers and n_out * n_in >= 4096:
        # 0.1 % of the entries x20: exercises the amax->scale clamp and fp8 saturation branches
        n_spike = max(1, (n_out * n_in) // 1000)
        idx = torch.randint(0, n_out * n_in, (n_spike,), generator=gen, device=device)
        w.view(-1)[idx] *= 20.0
    sd[name + ".weight"] = w.to(dtype)
    if bias:
        b = (torch.rand(n_out, generator=gen, device=device, dtype=torch.float32) * 2 - 1) / math.sqrt(n_in)
        sd[name + ".bias"] = b.to(dtype)


def _out_channels(params) -> int:
    """the predicted (noisy) channels: params.out_channels when set (FLUX.1 Fill / Depth / Canny), else in_channels"""
    out = getattr(params, "out_channels", None)
    return params.in_channels if out is None else out


def make_state_dict(params, seed: int = 0, dtype=torch.bfloat16, device="cpu") -> Dict[str, torch.Tensor]:
    """params: anything with the FluxParams fields (modules.flux_model.FluxParams)."""
    gen = torch.Generator(device=device).manual_seed(seed)
    H = params.hidden_size
    mlp = int(H * params.mlp_ratio)
    hd = H // params.num_heads
    sd: Dict[str, torch.Tensor] = {}
    L = lambda *a, **k: _linear(sd, *a, gen=gen, device=device, dtype=dtype, **k)
    L("img_in", H, params.in_channels)
    for emb, d_in in (("time_in", 256), ("vector_in", params.vec_in_dim)) + (
        (("guidance_in", 256),) if params.guidance_embed else ()
    ):
        L(emb + ".in_layer", H, d_in)
        L(emb + ".out_layer", H, H)
    L("txt_in", H, params.context_in_dim)

    def qk_scales(prefix):
        for nm in ("query_norm", "key_norm"):
            s = 1.0 + 0.1 * torch.randn(hd, generator=gen, device=device, dtype=torch.float32)
            sd[f"{prefix}.{nm}.scale"] = s.to(dtype)

    for i in range(params.depth):
        p = f"double_blocks.{i}"
        for s in ("img", "txt"):
            L(f"{p}.{s}_mod.lin", 6 * H, H, gain=0.5)
            L(f"{p}.{s}_attn.qkv", 3 * H, H, bias=params.qkv_bias)
            qk_scales(f"{p}.{s}_attn.norm")
            L(f"{p}.{s}_attn.proj", H, H)
            L(f"{p}.{s}_mlp.0", mlp, H)
            L(f"{p}.{s}_mlp.2", H, mlp)
    for i in range(params.depth_single_blocks):
        p = f"single_blocks.{i}"
        L(f"{p}.linear1", 3 * H + mlp, H)
        L(f"{p}.linear2", H, H + mlp)
        qk_scales(f"{p}.norm")
        L(f"{p}.modulation.lin", 3 * H, H, gain=0.5)
    L("final_layer.linear", _out_channels(params), H)
    L("final_layer.adaLN_modulation.1", 2 * H, H, gain=0.5)
    return sd


def make_inputs(params, height: int, width: int, txt_len: int, batch: int = 1, seed: int = 0,
                dtype=torch.bfloat16, real_tokens: int = 32):
    """Seeded request tensors: packed N(0,1) latent noise (the predicted channels only), T5-like `txt` whose rows
    >= real_tokens repeat one "pad" row, CLIP-like pooled `y`, position ids per
    flux_pipeline.py:280-292 / flux_emphasis.py:433-439.  All on CPU in the flow dtype."""
    gen = torch.Generator().manual_seed(1000 + seed)
    h2, w2 = math.ceil(height / 16), math.ceil(width / 16)
    img = torch.randn(batch, h2 * w2, _out_channels(params), generator=gen).to(dtype)
    txt = 0.1 * torch.randn(batch, txt_len, params.context_in_dim, generator=gen)
    if txt_len > real_tokens:
        txt[:, real_tokens:] = txt[:, real_tokens:real_tokens + 1]
    txt = txt.to(dtype)
    y = torch.randn(batch, params.vec_in_dim, generator=gen).to(dtype)
    img_ids = torch.zeros(h2, w2, 3, dtype=dtype)
    img_ids[..., 1] += torch.arange(h2, dtype=dtype)[:, None]
    img_ids[..., 2] += torch.arange(w2, dtype=dtype)[None, :]
    img_ids = img_ids[None].repeat(batch, 1, 1, 1).flatten(1, 2)
    txt_ids = torch.zeros(batch, txt_len, 3, dtype=dtype)
    return dict(img=img, img_ids=img_ids, txt=txt, txt_ids=txt_ids, y=y)


def make_controlnet_state_dict(params, num_double: int, num_single: int, num_mode: int = 0, seed: int = 0, guidance_embed=None,
                               dtype=torch.bfloat16, device="cpu", proj_gain: float = 1.0) -> Dict[str, torch.Tensor]:
    """A synthetic FLUX ControlNet for the main model of `params` under modules.controlnet.FluxControlNet's (BFL-style) key names: a trunk of
    `num_double` + `num_single` blocks like make_state_dict's (no final layer), controlnet_x_embedder, one controlnet_blocks /
    controlnet_single_blocks projection per block and, with `num_mode`, the controlnet_mode_embedder table.  Real checkpoints zero-initialise the
    projections before training; these are drawn like every other linear (`proj_gain`), so that the net's residuals are as large as the stream
    they join and a parity test cannot pass by ignoring them."""
    import copy

    p = copy.copy(params)
    p.depth, p.depth_single_blocks = int(num_double), int(num_single)
    if guidance_embed is not None:
        p.guidance_embed = bool(guidance_embed)
    sd = {k: v for k, v in make_state_dict(p, seed=seed + 7919, dtype=dtype, device=device).items() if not k.startswith("final_layer.")}
    gen = torch.Generator(device=device).manual_seed(seed + 104729)
    H = params.hidden_size
    L = lambda *a, **k: _linear(sd, *a, gen=gen, device=device, dtype=dtype, **k)
    L("controlnet_x_embedder", H, params.in_channels, gain=proj_gain)
    for i in range(num_double):
        L(f"controlnet_blocks.{i}", H, H, gain=proj_gain)
    for i in range(num_single):
        L(f"controlnet_single_blocks.{i}", H, H, gain=proj_gain)
    if num_mode:
        sd["controlnet_mode_embedder.weight"] = torch.randn(num_mode, H, generator=gen, device=device, dtype=torch.float32).to(dtype)
    return sd


def make_ip_adapter_state_dict(hidden: int, depth: int, num_tokens: int = 4, seed: int = 0, dtype=torch.bfloat16, device="cpu",
                               kv_gain: float = 4.0) -> Dict[str, torch.Tensor]:
    """A synthetic XLabs-format FLUX IP-Adapter (modules.ip_adapter): ip_adapter_proj_model.{proj, norm} and, per double block, the
    processor's ip_adapter_double_stream_{k,v}_proj.  `kv_gain` makes keys / values as large as a normalised query row (unit rms x 4), so
    the softmax is not flat and the term is as large as the stream it joins: a parity test cannot pass by ignoring it."""
    gen = torch.Generator(device=device).manual_seed(seed + 15485863)
    sd: Dict[str, torch.Tensor] = {}
    L = lambda *a, **k: _linear(sd, *a, gen=gen, device=device, dtype=dtype, **k)
    L("ip_adapter_proj_model.proj", num_tokens * 4096, 768, outliers=False)
    sd["ip_adapter_proj_model.norm.weight"] = (1.0 + 0.1 * torch.randn(4096, generator=gen, device=device)).to(dtype)
    sd["ip_adapter_proj_model.norm.bias"] = (0.1 * torch.randn(4096, generator=gen, device=device)).to(dtype)
    for i in range(depth):
        for kv in ("k", "v"):
            L(f"double_blocks.{i}.processor.ip_adapter_double_stream_{kv}_proj", hidden, 4096, gain=kv_gain, outliers=False)
    return sd


def make_clip_vision_state_dict(config: dict, seed: int = 0, dtype=torch.float32) -> Dict[str, torch.Tensor]:
    """A synthetic transformers CLIPVisionModelWithProjection state dict for a CLIPVisionConfig dict (hidden_size, intermediate_size,
    num_hidden_layers, num_attention_heads, image_size, patch_size, projection_dim): weights drawn so that activations stay O(1) through
    the depth (LayerNorm gains around 1, linears at 1 / sqrt(fan_in))."""
    gen = torch.Generator().manual_seed(seed + 32452843)
    D, Fd, P, S = config["hidden_size"], config["intermediate_size"], config["patch_size"], config["image_size"]
    n_pos = (S // P) ** 2 + 1
    rn = lambda *shape, s=1.0: (s * torch.randn(*shape, generator=gen)).to(dtype)
    sd = {"vision_model.embeddings.class_embedding": rn(D, s=0.5),
          "vision_model.embeddings.patch_embedding.weight": rn(D, config.get("num_channels", 3), P, P, s=1.0 / math.sqrt(3 * P * P)),
          "vision_model.embeddings.position_embedding.weight": rn(n_pos, D, s=0.1)}

    def ln(name):
        sd[name + ".weight"] = (1.0 + 0.1 * torch.randn(D, generator=gen)).to(dtype)
        sd[name + ".bias"] = rn(D, s=0.05)

    def lin(name, n_out, n_in, bias=True):
        sd[name + ".weight"] = rn(n_out, n_in, s=1.0 / math.sqrt(n_in))
        if bias:
            sd[name + ".bias"] = rn(n_out, s=0.05)

    ln("vision_model.pre_layrnorm")
    for i in range(config["num_hidden_layers"]):
        p = f"vision_model.encoder.layers.{i}"
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            lin(f"{p}.self_attn.{n}", D, D)
        ln(p + ".layer_norm1")
        ln(p + ".layer_norm2")
        lin(p + ".mlp.fc1", Fd, D)
        lin(p + ".mlp.fc2", D, Fd)
    ln("vision_model.post_layernorm")
    lin("visual_projection", config["projection_dim"], D, bias=False)
    return sd


def make_rrdbnet_state_dict(num_block: int = 2, nf: int = 64, gc: int = 32, scale: int = 4, seed: int = 0,
                            layout: str = "new") -> Dict[str, torch.Tensor]:
    """A seeded RRDBNet checkpoint (modules/upscaler.py) for tests and tools: Conv2d weights [Cout, Cin, 3, 3] and biases as fp32 tensors that
    hold bf16 values.  He-style gains keep the activations O(1) through a few blocks, so no branch can be ignored by a test: std 1.4 /
    sqrt(9 Cin) on the trunk's convolutions (the dense blocks, conv_body, conv_up1 / 2, conv_hr), 1.0 / sqrt(9 Cin) on conv_first and
    conv_last; biases N(0, 0.1).  `scale` 4 / 2 / 1 gives conv_first 3 / 12 / 48 input channels (Real-ESRGAN's pixel_unshuffle heads).
    `layout`: "new" (BasicSR keys) or "old" (the original ESRGAN x4 keys: model.0, model.1.sub.{i}.RDB{j}.conv{k}.0, model.1.sub.{n},
    model.3 / 6 / 8 / 10; scale 4 only)."""
    if scale not in (4, 2, 1):
        raise ValueError(f"make_rrdbnet_state_dict: scale={scale} must be 4, 2 or 1")
    if layout not in ("new", "old") or (layout == "old" and scale != 4):
        raise ValueError(f"make_rrdbnet_state_dict: layout={layout!r} must be 'new' or 'old' (old: scale 4 only)")
    gen = torch.Generator().manual_seed(1000 + seed)
    in_ch = {4: 3, 2: 12, 1: 48}[scale]
    sd: Dict[str, torch.Tensor] = {}

    def conv(name, co, ci, gain):
        sd[name + ".weight"] = (torch.randn(co, ci, 3, 3, generator=gen) * (gain / math.sqrt(9 * ci))).bfloat16().float()
        sd[name + ".bias"] = (0.1 * torch.randn(co, generator=gen)).bfloat16().float()

    conv("conv_first", nf, in_ch, 1.0)
    for i in range(num_block):
        for j in (1, 2, 3):
            for k in (1, 2, 3, 4, 5):
                conv(f"body.{i}.rdb{j}.conv{k}", nf if k == 5 else gc, nf + (k - 1) * gc, 1.4)
    for name in ("conv_body", "conv_up1", "conv_up2", "conv_hr"):
        conv(name, nf, nf, 1.4)
    conv("conv_last", 3, nf, 1.0)
    if layout == "new":
        return sd
    fixed = {"conv_first": "model.0", "conv_body": f"model.1.sub.{num_block}", "conv_up1": "model.3", "conv_up2": "model.6", "conv_hr": "model.8",
             "conv_last": "model.10"}
    old = {}
    for k, v in sd.items():
        base, leaf = k.rsplit(".", 1)
        if base in fixed:
            old[f"{fixed[base]}.{leaf}"] = v
        else:
            _, i, rdb, cv = base.split(".")
            old[f"model.1.sub.{i}.RDB{rdb[3:]}.conv{cv[4:]}.0.{leaf}"] = v
    return old


# the Depth Anything geometries of the three released sizes (LiheYoung/depth-anything-{small,base,large}-hf and the V2 checkpoints)
DEPTH_ANYTHING_SIZES = {
    "small": dict(hidden_size=384, num_attention_heads=6, num_hidden_layers=12, out_indices=[3, 6, 9, 12], neck_hidden_sizes=[48, 96, 192, 384],
                  fusion_hidden_size=64),
    "base": dict(hidden_size=768, num_attention_heads=12, num_hidden_layers=12, out_indices=[3, 6, 9, 12], neck_hidden_sizes=[96, 192, 384, 768],
                 fusion_hidden_size=128),
    "large": dict(hidden_size=1024, num_attention_heads=16, num_hidden_layers=24, out_indices=[5, 12, 18, 24],
                  neck_hidden_sizes=[256, 512, 1024, 1024], fusion_hidden_size=256),
}


def depth_anything_config(size: str = "large", **over) -> dict:
    """the config.json of a Depth Anything checkpoint of that size, as a dict (DepthAnythingConfig with an inline Dinov2Config)"""
    g = dict(DEPTH_ANYTHING_SIZES[size])
    g.update(over)
    bc = dict(model_type="dinov2", hidden_size=g["hidden_size"], num_attention_heads=g["num_attention_heads"],
              num_hidden_layers=g["num_hidden_layers"], image_size=518, patch_size=14, out_indices=list(g["out_indices"]), apply_layernorm=True,
              reshape_hidden_states=False, mlp_ratio=4, layerscale_value=1.0)
    return dict(model_type="depth_anything", backbone_config=bc, reassemble_hidden_size=g["hidden_size"], reassemble_factors=[4, 2, 1, 0.5],
                neck_hidden_sizes=list(g["neck_hidden_sizes"]), fusion_hidden_size=g["fusion_hidden_size"], head_hidden_size=g.get("head_hidden_size", 32),
                patch_size=14, depth_estimation_type="relative")


def make_depth_anything_state_dict(config: dict, seed: int = 0, dtype=torch.float32) -> Dict[str, torch.Tensor]:
    """A synthetic transformers DepthAnythingForDepthEstimation state dict for a config.json dict (depth_anything_config; the tests' tiny
    geometry).  transformers' own initialisation (std 0.02 everywhere) gives a depth of about 4e-5 that the last ReLU mostly zeroes; here
    every layer preserves variance instead, so that each branch reaches the output at O(1): linears and 1 x 1 convolutions at 1 /
    sqrt(fan_in), convolutions in front of a ReLU'd consumer at sqrt(2 / fan_in), LayerNorm gains around 1, LayerScale 0.3 +- 0.1 (non-zero:
    both residual branches count), and a head whose last convolution has non-negative weights and a positive bias, so that the depth is
    positive nearly everywhere and still varies over the image."""
    gen = torch.Generator().manual_seed(seed + 49979687)
    bc = config["backbone_config"]
    D, P = bc["hidden_size"], bc.get("patch_size", 14)
    Fd, n_pos = int(D * bc.get("mlp_ratio", 4)), (bc.get("image_size", 518) // P) ** 2 + 1
    Fh, Hh = config["fusion_hidden_size"], config.get("head_hidden_size", 32)
    rn = lambda *shape, s=1.0: (s * torch.randn(*shape, generator=gen)).to(dtype)  # noqa: E731
    sd = {}

    def ln(name):
        sd[name + ".weight"] = (1.0 + 0.1 * torch.randn(D, generator=gen)).to(dtype)
        sd[name + ".bias"] = rn(D, s=0.05)

    def lin(name, n_out, n_in):
        sd[name + ".weight"] = rn(n_out, n_in, s=1.0 / math.sqrt(n_in))
        sd[name + ".bias"] = rn(n_out, s=0.05)

    def conv(name, n_out, n_in, k, gain=1.0, bias=True):
        sd[name + ".weight"] = rn(n_out, n_in, k, k, s=gain / math.sqrt(n_in * k * k))
        if bias:
            sd[name + ".bias"] = rn(n_out, s=0.05)

    e = "backbone.embeddings."
    sd[e + "cls_token"] = rn(1, 1, D, s=0.5)
    sd[e + "mask_token"] = torch.zeros(1, D, dtype=dtype)
    sd[e + "position_embeddings"] = rn(1, n_pos, D, s=0.1)
    conv(e + "patch_embeddings.projection", D, 3, P)
    for i in range(bc["num_hidden_layers"]):
        p = f"backbone.encoder.layer.{i}."
        ln(p + "norm1")
        for n in ("query", "key", "value"):
            lin(p + f"attention.attention.{n}", D, D)
        lin(p + "attention.output.dense", D, D)
        sd[p + "layer_scale1.lambda1"] = (0.3 + 0.1 * torch.randn(D, generator=gen)).to(dtype)
        ln(p + "norm2")
        lin(p + "mlp.fc1", Fd, D)
        lin(p + "mlp.fc2", D, Fd)
        sd[p + "layer_scale2.lambda1"] = (0.3 + 0.1 * torch.randn(D, generator=gen)).to(dtype)
    ln("backbone.layernorm")
    g2 = math.sqrt(2.0)
    for i, (ch, f) in enumerate(zip(config["neck_hidden_sizes"], config.get("reassemble_factors", [4, 2, 1, 0.5]))):
        p = f"neck.reassemble_stage.layers.{i}."
        conv(p + "projection", ch, D, 1)
        if f > 1:  # ConvTranspose2d weight [Cin, Cout, f, f]: every output pixel sums Cin products
            sd[p + "resize.weight"] = rn(ch, ch, int(f), int(f), s=1.0 / math.sqrt(ch))
            sd[p + "resize.bias"] = rn(ch, s=0.05)
        elif f < 1:
            conv(p + "resize", ch, ch, 3)
        conv(f"neck.convs.{i}", Fh, ch, 3, bias=False)
        q = f"neck.fusion_stage.layers.{i}."
        conv(q + "projection", Fh, Fh, 1)
        for n in ("residual_layer1", "residual_layer2"):
            conv(f"{q}{n}.convolution1", Fh, Fh, 3, gain=g2)   # reads relu(x)
            conv(f"{q}{n}.convolution2", Fh, Fh, 3, gain=0.5 * g2)  # the residual branch at half the stream's size
    conv("head.conv1", Fh // 2, Fh, 3)
    conv("head.conv2", Hh, Fh // 2, 3)
    sd["head.conv3.weight"] = (torch.rand(1, Hh, 1, 1, generator=gen) * (2.0 / Hh)).to(dtype)
    sd["head.conv3.bias"] = torch.full((1,), 0.25, dtype=dtype)
    return sd
