"""Helpers of tests/test_fbcache_gpu.py: the first-block step-cache rule written out in torch around the engine's phase
hook -- every forward piece runs on the engine's own buffers (fluxmi_engine_run_phase), everything the rule adds (snapshot, residual, ratio in
fp64, decision, apply, the update) is torch bf16 arithmetic on tensors read and written with fluxmi_engine_copy_buffer."""
import math

import torch


def eng_read(model, name, shape, dtype=torch.bfloat16):
    from fluxmi import _lib, ops

    out = torch.empty(shape, dtype=dtype, device="cuda")
    _lib.call("fluxmi_engine_copy_buffer", model._engine, name.encode(), 0, ops._p(out), out.numel() * out.element_size(), 0, ops._stream())
    return out


def eng_write(model, name, t):
    from fluxmi import _lib, ops

    t = t.contiguous()
    _lib.call("fluxmi_engine_copy_buffer", model._engine, name.encode(), 0, ops._p(t), t.numel() * t.element_size(), 1, ops._stream())
    torch.cuda.synchronize()  # `t` may be a temporary


def run_phase(model, mode, p0, p1, step=-1):
    from fluxmi import _lib, ops

    _lib.call("fluxmi_engine_run_phase", model._engine, mode, p0, p1, step, ops._stream())


def decide(ratios, have_full, consec, threshold, max_hits):
    """the host's rule: a hit needs a full step behind it in this call, every sample under the threshold, and room under the hit bound"""
    return bool(have_full and (max_hits <= 0 or consec < max_hits) and all(r < threshold for r in ratios))


def python_cached_loop(model, stream, ts, mode, threshold, max_hits, Lt, Lpred, scale=None):
    """The cached denoise loop on the engine's buffers, to be called right after a Flux.denoise call of the same request (it left the
    embedded text, the request's conditioning and the modulation table of `ts`).  stream: the caller's samples [B, Li, C_in] (Kontext: the
    reference rows behind the Lpred noisy rows; Fill: the conditioning channels behind the C_out noisy ones), stepped in place like the
    engine's own copy.  scale: the true-CFG scale of a guided request (the engine then holds 2B samples).  Returns (stream, ratios, hits)."""
    B, Li, C_in = stream.shape
    Be = 2 * B if scale is not None else B
    H, C_out = model.hidden_size, model.out_channels
    L = Lt + Li
    x = stream.clone()
    r_ref = R = None
    have_full, consec, log_r, log_h = False, 0, [], []
    with model._lock:
        for i, (t_curr, t_prev) in enumerate(zip(ts[:-1], ts[1:])):
            eng_write(model, "img_s", torch.cat((x, x), 0) if scale is not None else x)
            run_phase(model, mode, 0, 0, step=i)
            h0 = eng_read(model, "x", (Be, L, H))[:, Lt:Lt + Lpred].clone()
            run_phase(model, mode, 1, 1)
            xs = eng_read(model, "x", (Be, L, H))
            h1 = xs[:, Lt:Lt + Lpred].clone()
            r = h1 - h0
            assert r.dtype == torch.bfloat16
            if have_full:
                ratios = [((r[b].double() - r_ref[b].double()).abs().sum() / r_ref[b].double().abs().sum()).item() for b in range(Be)]
            else:
                ratios = [math.inf] * Be
            hit = decide(ratios, have_full, consec, threshold, max_hits)
            log_r.append(ratios)
            log_h.append(hit)
            consec = consec + 1 if hit else 0
            if hit:
                xs[:, Lt:Lt + Lpred] = h1 + R
                eng_write(model, "x", xs)
            else:
                have_full = True
                r_ref = r
                run_phase(model, mode, 2, 2)
                R = eng_read(model, "x", (Be, L, H))[:, Lt:Lt + Lpred] - h1
            run_phase(model, mode, 3, 3)
            pred = eng_read(model, "pred_s", (Be, Lpred, C_out))
            if scale is not None:
                c, u = pred[:B], pred[B:]
                pred = u + scale * (c - u)
            x[:, :Lpred, :C_out] = x[:, :Lpred, :C_out] + (t_prev - t_curr) * pred
    return x, torch.tensor(log_r, dtype=torch.float64), log_h


def clearance(ratios, hits, threshold):
    """smallest relative distance of a decided ratio from the threshold over the steps whose decision the threshold made (finite ratios)"""
    vals = [abs(r - threshold) / threshold for row in ratios.tolist() for r in row if math.isfinite(r)]
    return min(vals) if vals else math.inf
