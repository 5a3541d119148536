"""The native JPEG encoder (csrc/jpeg.hip) beside today's path at a request's size: from decoded pixels on the device ([B, 3, H, W] floats in
[-1, 1], what the VAE returns) to the file's bytes on the host.
    python tools/jpeg_step.py [--sizes 1024 4096] [--rounds 7] [--out profiles/jpeg.txt]
"pil" is FluxPipeline.to_uint8 (its device-to-host copy included) + FluxPipeline._jpeg; "native" is to_uint8_device + fluxmi.ops.jpeg_encode
(two copies back: the length, then that many bytes).  Both run in ONE process, alternating, `rounds` times each after a warm-up; median, min and
max of a host clock are printed.  Inputs: "photo" (smooth structure under mild noise) and "noise" (uniform).  Also: the file sizes, whether the
two files decode to the same pixels, the cost in bytes of the default restart interval against none, and one whole generate() of each kind on
the small synthetic model of the tests.  Prints one JSON line per figure, and writes them to --out when given.  For the kernels' own durations:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/jpeg_step.py --kernels-only --sizes 1024 4096"""
import argparse
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "flux-fp8-api_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT):
    sys.path.insert(0, p)
import numpy as np
import torch


def photo_like(n, seed=0):
    """float32 [1, 3, n, n] in [-1, 1]: low-frequency structure, a few hard edges, sensor-like noise"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(n, dtype=torch.float32), torch.arange(n, dtype=torch.float32), indexing="ij")
    ch = []
    for c in range(3):
        v = 0.5 * torch.sin(xx / (37.0 + 11 * c) + yy / (53.0 - 9 * c)) + 0.3 * torch.cos(yy / (19.0 + 5 * c)) * torch.sin(xx / 91.0)
        v += 0.25 * ((xx // (n // 8) + yy // (n // 6)) % 2) - 0.1
        ch.append(v + 0.02 * torch.randn(n, n, generator=g))
    return torch.stack(ch)[None].clamp(-1, 1)


def noise(n, seed=1):
    return torch.rand(1, 3, n, n, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def stats(t):
    return dict(median_ms=round(float(np.median(t)), 3), min_ms=round(min(t), 3), max_ms=round(max(t), 3))


def alternate(fns: dict, rounds: int):
    """every fn once to warm up, then `rounds` rounds of every fn in turn, each timed on the host clock around a synchronise"""
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
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kernels-only", action="store_true", help="a few native encodes per size and nothing else (for a kernel trace)")
    ap.add_argument("--no-generate", action="store_true", help="skip the whole-request figures")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("jpeg_step: needs the GPU")
    from PIL import Image

    from flux_pipeline import FluxPipeline
    from fluxmi import ops

    dev = torch.device("cuda:0")
    lines = []

    def say(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    for n in a.sizes:
        for kind, make in (("photo", photo_like), ("noise", noise)):
            x = make(n).to(dev)
            if a.kernels_only:
                px = FluxPipeline.to_uint8_device(x)
                for _ in range(3):
                    ops.jpeg_encode(px, 99)
                torch.cuda.synchronize()
                continue
            for q in (99, 90):
                pil = lambda: FluxPipeline._jpeg(FluxPipeline.to_uint8(x), q).getvalue()
                native = lambda: ops.jpeg_encode(FluxPipeline.to_uint8_device(x), q)
                f_pil, f_nat = pil(), native()
                same = bool(np.array_equal(np.asarray(Image.open(io.BytesIO(f_pil))), np.asarray(Image.open(io.BytesIO(f_nat)))))
                t = alternate({"pil": pil, "native": native}, a.rounds)
                say(what="pixels on the device -> bytes on the host", size=n, input=kind, quality=q, pil=t["pil"], native=t["native"],
                    pil_bytes=len(f_pil), native_bytes=len(f_nat), decode_to_the_same_pixels=same,
                    speedup_median=round(t["pil"]["median_ms"] / t["native"]["median_ms"], 2))
            if n <= 1024:
                px = FluxPipeline.to_uint8_device(x)
                r0, rd = len(ops.jpeg_encode(px, 99, restart_interval=0)), len(ops.jpeg_encode(px, 99))
                say(what="default restart interval (4 MCUs at 4:2:0) against none", size=n, input=kind, quality=99, bytes_R0=r0, bytes_default=rd,
                    overhead_percent=round(100.0 * (rd - r0) / r0, 3))
    if not (a.kernels_only or a.no_generate):
        from test_cfg_gpu import prompts, tiny_pipeline

        pipe = tiny_pipeline(dev)
        pipe.compile()
        pos, _ = prompts()
        kw = dict(width=512, height=512, num_steps=4, seed=7, silent=True)
        t = alternate({enc: (lambda enc=enc: pipe.generate(pos, jpeg_encoder=enc, **kw)) for enc in ("pil", "native")}, a.rounds)
        say(what="one whole generate(): the tests' small synthetic model, 512 x 512, 4 steps", pil=t["pil"], native=t["native"])
    if a.out and lines:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
