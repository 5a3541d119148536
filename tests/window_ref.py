"""A torch restatement, on CPU tensors, of the windowed update's definition (include/fluxmi.h, fluxmi_window_gather / fluxmi_window_step):
fp32 operations one by one, `.bfloat16()` wherever the formula rounds.  The canvas is bf16 [N, Hc, Wc, C]; the stream holds S = N * ny * nx
windows of h x w tokens (2S when guided: the negative branches behind the prompt branches), sample (n * ny + a) * nx + b window (a, b) of
image n at canvas token (row0[a], col0[b])."""
import torch


def rb(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 (round to nearest even) -> fp32"""
    return x.bfloat16().float()


def gather(canvas: torch.Tensor, row0, col0, h: int, w: int, guided: bool = False) -> torch.Tensor:
    """the stream of the canvas: bf16 [S or 2S, h * w, C]"""
    N, Hc, Wc, C = canvas.shape
    out = [canvas[n, r:r + h, c:c + w].reshape(h * w, C) for n in range(N) for r in row0 for c in col0]
    out = torch.stack(out, 0)
    return torch.cat((out, out), 0) if guided else out


def guided_velocity(pred: torch.Tensor, scale: float) -> torch.Tensor:
    """fluxmi_cfg_euler's bf16 chain d, m, p on the two halves of pred -> fp32 values of bf16 [S, ...]"""
    S = pred.shape[0] // 2
    c, u = pred[:S].float(), pred[S:].float()
    s = torch.tensor(scale, dtype=torch.float32)
    d = rb(c - u)
    m = rb(s * d)
    return rb(u + m)


def step(canvas: torch.Tensor, pred: torch.Tensor, dt: float, row0, col0, Ny: torch.Tensor, Nx: torch.Tensor, h: int, w: int, scale=None):
    """-> (the new canvas bf16 [N, Hc, Wc, C], the new stream bf16 like pred).  dt, scale: the fp32 values the kernel reads."""
    N, Hc, Wc, C = canvas.shape
    ny, nx = len(row0), len(col0)
    v = pred.float() if scale is None else guided_velocity(pred, scale)
    v = v.reshape(N, ny, nx, h, w, C)
    num = torch.zeros(N, Hc, Wc, C, dtype=torch.float32)
    for a in range(ny):  # ascending (a, b): the order of the fp32 sum
        for b in range(nx):
            r, c = row0[a], col0[b]
            wgt = Ny[a, r:r + h].float()[:, None] * Nx[b, c:c + w].float()[None, :]  # fp32 product, rounded
            prod = wgt[None, :, :, None] * v[:, a, b]                                 # fp32 product, rounded
            num[:, r:r + h, c:c + w] = num[:, r:r + h, c:c + w] + prod               # fp32 sum, rounded
    vbar = rb(num)
    dtf = torch.tensor(dt, dtype=torch.float32)
    x = (canvas.float() + rb(dtf * vbar)).bfloat16()
    return x, gather(x, row0, col0, h, w, guided=scale is not None)
