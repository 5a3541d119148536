"""The native image resampler (csrc/resample.hip) beside today's path at the sizes requests use: from an RGB uint8 array on the host to the
resized uint8 image on the device.
    python tools/resize_step.py [--rounds 7] [--out profiles/resize.txt]
"pil" is host array -> PIL.Image.resize -> upload; "native" is host array -> upload (pinned) -> fluxmi.ops.resize_u8; "native_device" is
ops.resize_u8 alone on pixels already on the device (what an upscaled init image or a second resize of the same request pays).  All run in ONE
process, alternating, `rounds` times each after a warm-up; median, min and max of a host clock around a synchronise.  Also: whether the two
results are equal, each case's byte bound (bytes read + bytes written at the device's measured copy rate) and which launches ran.  One JSON
line per figure, written to --out when given.  For the kernels' own durations:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/resize_step.py --kernels-only"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flux-fp8-api_amd"))
import numpy as np
import torch

CASES = [((4096, 4096), (1024, 1024), "lanczos"), ((4096, 4096), (1024, 1024), "bicubic"), ((768, 1024), (1024, 1024), "lanczos"),
         ((768, 768), (384, 384), "bicubic")]  # (H, W) -> (h, w); the last is SigLIP's


def photo_like(H, W, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    ch = [0.5 + 0.3 * np.sin(xx / (37 + 11 * c) + yy / (53 - 9 * c)) + 0.15 * ((xx // 97 + yy // 61) % 2) for c in range(3)]
    return np.clip((np.stack(ch, -1) + 0.02 * rng.standard_normal((H, W, 3))) * 255, 0, 255).astype(np.uint8)


def stats(t):
    return dict(median_ms=round(float(np.median(t)), 3), min_ms=round(min(t), 3), max_ms=round(max(t), 3))


def alternate(fns: dict, rounds: int):
    times = {k: [] for k in fns}
    for r in range(rounds + 1):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: stats(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kernels-only", action="store_true", help="a few native resizes per case and nothing else (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("resize_step: needs the GPU")
    from PIL import Image

    from fluxmi import ops

    dev = torch.device("cuda:0")
    pil_filter = {"lanczos": Image.LANCZOS, "bicubic": Image.BICUBIC}
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    if not a.kernels_only:  # the device's copy rate: a 256 MiB device-to-device copy, bytes read + written per second
        src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        rate = 2 * src.numel() / (alternate({"copy": lambda: dst.copy_(src)}, 7)["copy"]["median_ms"] * 1e-3)
        emit(figure="copy_rate", GBps=round(rate / 1e9, 1))
        del src, dst
    for (H, W), (h, w), filt in CASES:
        host = photo_like(H, W)
        pinned = torch.from_numpy(host).pin_memory()
        on_dev = torch.from_numpy(host).to(dev)[None]
        fused, work = ops.resample_plan(1, H, W, 3, h, w, filt)
        case = f"{W}x{H}->{w}x{h} {filt}"
        if a.kernels_only:
            for _ in range(5):
                ops.resize_u8(on_dev, (w, h), filt)
            torch.cuda.synchronize()
            continue
        fns = {
            "pil": lambda: torch.from_numpy(np.asarray(Image.fromarray(host).resize((w, h), pil_filter[filt]))).to(dev),
            "native": lambda: ops.resize_u8(pinned.to(dev, non_blocking=True)[None], (w, h), filt),
            "native_device": lambda: ops.resize_u8(on_dev, (w, h), filt),
        }
        equal = bool(torch.equal(fns["pil"](), fns["native"]()[0]))
        t = alternate(fns, a.rounds)
        nbytes = 3 * (H * W + h * w)
        emit(figure="resize", case=case, equal_to_pil=equal, launches="fused" if fused else "horizontal + vertical" if (H != h and W != w) else "one pass", workspace_bytes=work,
             bytes_moved=nbytes, byte_bound_ms=round(nbytes / rate * 1e3, 4), **{k: v for k, v in t.items()})
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
