"""Helpers of tests/test_inpaint_gpu.py and tests/test_inpaint_cpu.py: the masked-latent inpainting update written out in torch.

    x1 = x + dt * v                                  (guided: x + dt * (u + s * (c - u)))
    p  = t_next * noise + (1.0 - t_next) * x0
    x' = (1 - m) * p + m * x1

on bf16 tensors with python scalars (every operation rounds to bf16 once, the scalars enter as fp32), and the same thing as an explicit fp32
model with the roundings written out (csrc/update_step.hip, the BLEND arms of euler_kernel)."""
import torch


def effective_mask(m, thr=None):
    """differential diffusion: the binary mask of a step, compared in fp32 against the fp32 threshold (strict)"""
    if thr is None:
        return m
    return (m.float() > torch.tensor(thr, dtype=torch.float32, device=m.device)).to(m.dtype)


def blend(x1, x0, noise, m, t_next, thr=None):
    """the blend behind an update: python scalars on bf16 tensors"""
    m = effective_mask(m, thr)
    p = t_next * noise + (1.0 - t_next) * x0
    return (1 - m) * p + m * x1


def blend_step(x, v, dt, t_next, x0, noise, m, thr=None, scale=None):
    """one masked step; v = the prediction, or (c, u) with `scale` for the guided update"""
    if scale is None:
        x1 = x + dt * v
    else:
        c, u = v
        x1 = x + dt * (u + scale * (c - u))
    return blend(x1, x0, noise, m, t_next, thr)


def rbf(t):
    """one bf16 rounding of an fp32 tensor, kept in fp32"""
    return t.to(torch.bfloat16).float()


def blend_step_fp32_model(x, v, dt, t_next, x0, noise, m, thr=None):
    """the unguided masked step as the kernel computes it: fp32 operands, t_next and 1.0 - t_next (subtracted in double) each cast to fp32,
    one bf16 rounding behind every operation"""
    f32 = lambda s: torch.tensor(s, dtype=torch.float64).to(torch.float32)
    x, v, x0, noise, m = (t.float() for t in (x, v, x0, noise, m))
    if thr is not None:
        m = (m > f32(thr)).float()
    x1 = rbf(x + rbf(f32(dt) * v))
    p = rbf(rbf(f32(t_next) * noise) + rbf(f32(1.0 - t_next) * x0))
    return rbf(rbf(rbf(1.0 - m) * p) + rbf(m * x1)).to(torch.bfloat16)


def make_inpaint(B, Li, C, seed, device="cpu", mask_batch=1):
    """x0 / noise [B, Li, C] and a mixed mask [mask_batch, Li, C]: ~40 % zeros, ~40 % ones, the rest soft values in (0, 1)"""
    g = torch.Generator().manual_seed(9000 + seed)
    x0 = torch.randn(B, Li, C, generator=g).to(torch.bfloat16)
    noise = torch.randn(B, Li, C, generator=g).to(torch.bfloat16)
    r = torch.rand(mask_batch, Li, C, generator=g)
    m = torch.where(r < 0.4, torch.zeros_like(r), torch.where(r < 0.8, torch.ones_like(r), r)).to(torch.bfloat16)
    return x0.to(device), noise.to(device), m.to(device)
