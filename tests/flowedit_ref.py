"""References of FlowEdit (include/fluxmi.h: fluxmi_flowedit_couple / _step; fluxmi/flowedit.py), for tests/test_flowedit_cpu.py and
tests/test_flowedit_gpu.py.

  couple_bf16 / step_bf16   the torch restatement of the kernel: the bf16 chain as the header writes it -- one rounding per operation, the
                            scalars fp32, the accumulator fp32 with product and sum rounded separately -- with the normals passed in
  edit_fp64                 the whole algorithm (skipped, coupled and tail steps) in float64 on a caller-supplied velocity function
"""
import struct

import torch


def f32(v: float) -> float:
    """a python float rounded to fp32, as a device table holds it"""
    return struct.unpack("f", struct.pack("f", float(v)))[0]


def couple_bf16(z, x0, t, one_minus_t, normals):
    """z, x0 bf16 [B, ...]; normals fp32 of the same shape (fluxmi_philox_normal's); t, one_minus_t: the fp32 table values -> (zs, zt)"""
    assert z.dtype == torch.bfloat16 and x0.dtype == torch.bfloat16 and normals.dtype == torch.float32
    n = normals.to(torch.bfloat16)
    zs = f32(one_minus_t) * x0 + f32(t) * n   # bf16 tensors and python scalars: every product and the sum are rounded to bf16
    zt = (z + zs) - x0
    assert zs.dtype == torch.bfloat16 and zt.dtype == torch.bfloat16
    return zs, zt


def step_bf16(pred, z, acc, x0, row, ctl_row, normals):
    """One fluxmi_flowedit_step: pred bf16 [2B, ...] (source half, target half), z / x0 bf16 [B, ...], acc fp32 [B, ...] or None, row =
    (w, dt, tn, 1 - tn), ctl_row = (first, apply), normals fp32 [B, ...] of the NEXT draw -> (img [2B, ...], z', acc')."""
    B = z.shape[0]
    w, dt, tn, om = (f32(v) for v in row)
    first, apply = bool(ctl_row[0]), bool(ctl_row[1])
    vs, vt = pred[:B], pred[B:]
    d = vt - vs                                                   # bf16
    base = torch.zeros_like(d, dtype=torch.float32) if first else acc
    a = base + w * d.float()                                      # fp32: the product, then the sum
    assert a.dtype == torch.float32
    if apply:
        m = dt * a.to(torch.bfloat16)                             # bf16(dt * D)
        z = z + m                                                 # bf16(float(z) + float(m))
    zs, zt = couple_bf16(z, x0, tn, om, normals)
    return torch.cat((zs, zt), 0), z, a


def edit_fp64(x0, velocity, timesteps, n_max=None, n_min=0, n_avg=1, normal=None):
    """FlowEdit in float64.  velocity(x, t, branch) with branch "src" / "tar"; normal(k) -> the k-th draw (a tensor like x0), k counting
    couplings from 0 (default: seeded torch.randn).  Steps i with T - i > n_max are skipped, those with n_min < T - i <= n_max coupled
    (n_avg evaluations each at t_i, then z += (t_{i+1} - t_i) * mean(v_tar - v_src)), the rest an Euler tail on the target branch that
    starts from zt of one more coupling."""
    x0 = x0.double()
    ts = [float(t) for t in timesteps]
    T = len(ts) - 1
    n_max = T if n_max is None else n_max
    if normal is None:
        g = torch.Generator().manual_seed(0)
        normal = lambda k: torch.randn(x0.shape, generator=g, dtype=torch.float64)
    z = x0.clone()
    k = 0
    tail = None
    for i in range(T):
        left = T - i
        if left > n_max:
            continue
        t, tn = ts[i], ts[i + 1]
        if left > n_min:
            acc = torch.zeros_like(z)
            for _ in range(n_avg):
                zs = (1.0 - t) * x0 + t * normal(k).double()
                k += 1
                zt = z + zs - x0
                acc = acc + (velocity(zt, t, "tar") - velocity(zs, t, "src")) / n_avg
            z = z + (tn - t) * acc
        else:
            if tail is None:
                zs = (1.0 - t) * x0 + t * normal(k).double()
                k += 1
                tail = z + zs - x0
            tail = tail + (tn - t) * velocity(tail, t, "tar")
    return z if tail is None else tail
