"""Reference for the FLUX ControlNet tests: diffusers' FluxControlNetModel.forward and the residual insertion of
FluxTransformer2DModel.forward, RESTATED from oracle/flux_oracle.py's blocks (diffusers itself is not available offline, so parity with it is
unpinned: DESIGN.md section 7).  Two FluxOracles are composed:

  ControlNet (its own weights, BFL-style names, no final layer):
      h   = img_in(img) + controlnet_x_embedder(cond)
      txt = [controlnet_mode_embedder[mode] ;] txt_in(txt)          (Union: the mode row's position id is txt_ids[:1])
      after double block k:  Rd[k] = controlnet_blocks[k](h)
      after single block k:  Rs[k] = controlnet_single_blocks[k](x[:, Lt:])
  main model:
      after double block i:  img = img + Rd[i // ceil(depth / Nd)] * s
      after single block i:  x[:, Lt:] = x[:, Lt:] + Rs[i // ceil(depth_single / Ns)] * s

every operation on bf16 tensors with `s` a Python float, i.e. R = bf16(bf16(proj) * s) and bf16(img + R).  The controlnet_* linears are never
quantised."""
import math

import torch

import flux_oracle as fo


class ControlNetOracle(fo.FluxOracle):
    def _is_quantized(self, name: str) -> bool:
        if name.startswith("controlnet_"):
            return False
        return super()._is_quantized(name)

    def residuals(self, img, img_ids, txt, txt_ids, timesteps, y, guidance, cond, mode=None):
        """-> (Rd, Rs): the unscaled projections, lists of bf16 [B, Li, H]"""
        h = self.lin["img_in"](img) + self.lin["controlnet_x_embedder"](cond)
        vec = self.embed_vec(timesteps, y, guidance if self.p.guidance_embed else None)
        txt = self.lin["txt_in"](txt)
        if mode is not None:
            row = self.sd["controlnet_mode_embedder.weight"][mode].to(txt.dtype)
            txt = torch.cat((row[None, None].expand(txt.shape[0], 1, -1), txt), 1)
            txt_ids = torch.cat((txt_ids[:, :1], txt_ids), 1)
        pe = fo.rope_table(torch.cat((txt_ids, img_ids), 1), self.p.axes_dim, self.p.theta, self.dtype)
        Rd, Rs = [], []
        for i in range(self.p.depth):
            h, txt = self.double_block(i, h, txt, vec, pe)
            Rd.append(self.lin[f"controlnet_blocks.{i}"](h))
        x = torch.cat((txt, h), 1)
        for i in range(self.p.depth_single_blocks):
            x = self.single_block(i, x, vec, pe)
            Rs.append(self.lin[f"controlnet_single_blocks.{i}"](x[:, txt.shape[1]:]))
        return Rd, Rs


def make_net_oracle(net_sd, main_params: fo.FluxParams, quantize=None):
    """the oracle of a BFL-named ControlNet state dict for a main model of `main_params`: geometry read off the keys"""
    import dataclasses

    nd = len([k for k in net_sd if k.startswith("controlnet_blocks.") and k.endswith(".weight")])
    ns = len([k for k in net_sd if k.startswith("controlnet_single_blocks.") and k.endswith(".weight")])
    p = dataclasses.replace(main_params, depth=nd, depth_single_blocks=ns, guidance_embed="guidance_in.in_layer.weight" in net_sd)
    return ControlNetOracle({k: v.clone() for k, v in net_sd.items()}, p, quantize=quantize)


def block_index(i: int, n_blocks: int, n_res: int) -> int:
    return i // int(math.ceil(n_blocks / n_res))


def forward(main: fo.FluxOracle, net, img, img_ids, txt, txt_ids, timesteps, y, guidance, cond=None, mode=None, scale=1.0):
    """main.forward with the ControlNet's residuals inserted; net None (or cond None): main.forward itself, line for line"""
    Rd = Rs = []
    if net is not None and cond is not None:
        Rd, Rs = net.residuals(img, img_ids, txt, txt_ids, timesteps, y, guidance, cond, mode)
    s = float(scale)
    h = main.lin["img_in"](img)
    vec = main.embed_vec(timesteps, y, guidance)
    t = main.lin["txt_in"](txt)
    pe = fo.rope_table(torch.cat((txt_ids, img_ids), 1), main.p.axes_dim, main.p.theta, main.dtype)
    for i in range(main.p.depth):
        h, t = main.double_block(i, h, t, vec, pe)
        if Rd:
            h = h + Rd[block_index(i, main.p.depth, len(Rd))] * s
    Lt = t.shape[1]
    x = torch.cat((t, h), 1)
    for i in range(main.p.depth_single_blocks):
        x = main.single_block(i, x, vec, pe)
        if Rs:
            x = torch.cat((x[:, :Lt], x[:, Lt:] + Rs[block_index(i, main.p.depth_single_blocks, len(Rs))] * s), 1)
    return main.final_layer(x[:, Lt:], vec)


def denoise(main, net, img, img_ids, txt, txt_ids, y, timesteps, guidance=3.5, cond=None, mode=None, scale=1.0, keep=None):
    """fo.denoise over `forward`; keep[i] False: step i runs without the net"""
    B = img.shape[0]
    g = torch.full((B,), guidance, dtype=main.dtype)
    for i, (t_curr, t_prev) in enumerate(zip(timesteps[:-1], timesteps[1:])):
        t_vec = torch.full((B,), t_curr, dtype=main.dtype)
        on = keep is None or keep[i]
        pred = forward(main, net if on else None, img, img_ids, txt, txt_ids, t_vec, y, g, cond, mode, scale)
        img = img + (t_prev - t_curr) * pred
    return img
