"""The native PNG encoder (csrc/png.hip) beside Pillow at a request's size: from decoded pixels on the device ([B, 3, H, W] floats in
[-1, 1], what the VAE returns) to the file's bytes on the host.
    python tools/png_step.py [--sizes 1024 4096] [--rounds 5] [--out profiles/png.txt]
"pil1" / "pil6" are FluxPipeline.to_uint8 (its device-to-host copy included) + Pillow at compress_level 1 / 6 (6 is Pillow's default and the
pipeline's png_encoder="pil"); "native" is to_uint8_device + fluxmi.ops.png_encode (two copies back -- the length, then that many bytes --
and the host's CRC-32 pass, whose own time is reported).  All three run in ONE process, alternating, `rounds` times each after a warm-up;
median, min and max of a host clock.  Inputs: "photo" (smooth structure under mild noise) and "noise" (uniform).  Also the three file
sizes, the workspace size, and whether the native file decodes to the pixels.  One JSON line per figure, appended to --out when given.
For the kernels' own durations:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/png_step.py --kernels-only --sizes 1024 4096"""
import argparse
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "flux-fp8-api_amd"), os.path.join(ROOT, "tools"), ROOT):
    sys.path.insert(0, p)
import numpy as np
import torch

from jpeg_step import alternate, noise, photo_like


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true", help="a few native encodes per size and nothing else (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("png_step: needs the GPU")
    from PIL import Image

    from flux_pipeline import FluxPipeline
    from fluxmi import ops

    dev = torch.device("cuda:0")
    lines = []
    for n in a.sizes:
        for kind, make in (("photo", photo_like), ("noise", noise)):
            x = make(n).to(dev)
            if a.kernels_only:
                px = FluxPipeline.to_uint8_device(x)
                for _ in range(3):
                    ops.png_encode(px)
                torch.cuda.synchronize()
                continue

            def pil(level):
                buf = io.BytesIO()
                Image.fromarray(FluxPipeline.to_uint8(x)[0].numpy()).save(buf, format="PNG", compress_level=level)
                return buf.getvalue()

            prof = {}
            native = lambda: ops.png_encode(FluxPipeline.to_uint8_device(x), profile=prof)
            files = {"pil1": pil(1), "pil6": pil(6), "native": native()}
            lossless = bool(np.array_equal(np.asarray(Image.open(io.BytesIO(files["native"]))), FluxPipeline.to_uint8(x)[0].numpy()))
            crc = []
            t = alternate({"pil1": lambda: pil(1), "pil6": lambda: pil(6), "native": lambda: (native(), crc.append(prof["crc_ms"]))}, a.rounds)
            lines.append(json.dumps(dict(what="pixels on the device -> PNG bytes on the host", size=n, input=kind, **t,
                                         bytes={k: len(v) for k, v in files.items()}, native_decodes_to_the_pixels=lossless,
                                         native_host_crc_ms_median=round(float(np.median(crc[1:])), 3), native_work_bytes=prof["work_bytes"],
                                         speedup_vs_pil6_median=round(t["pil6"]["median_ms"] / t["native"]["median_ms"], 2))))
            print(lines[-1], flush=True)
    if a.out and lines:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
