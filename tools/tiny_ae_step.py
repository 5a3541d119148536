"""Time of one decode of a FLUX latent to pixels, three ways, in one process with the kinds ALTERNATING round after round (drift of the
device shows in every kind alike): synthetic weights, B = 1, a 1024^2 image (latent 128 x 128) unless told otherwise.
    vae       the autoencoder's decoder (modules/autoencoder.py), FLUX geometry
    unfused   the tiny decoder (modules/tiny_vae.py) with each residual block as THREE fluxmi_conv3x3_dense launches plus a torch add and
              ReLU: the building block this repository had before fluxmi_conv3x3_block, the baseline the fusion is judged by
    fused     the tiny decoder as shipped: one fluxmi_conv3x3_block launch per residual block
and, with --blocks, one residual block alone at 128^2 .. 1024^2 pixels, fused against unfused, 50 back-to-back calls per timing.  Device events around each
timed window, an untimed call of the same kind in front of every timed one.
    python tools/tiny_ae_step.py [--height 1024 --width 1024] [--rounds 5] [--kinds vae,unfused,fused] [--blocks]
Prints one JSON line per kind (and per block size): every round's ms, the median and the spread (max - min)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flux-fp8-api_amd"))
import torch

from fluxmi import ops, synth
from modules.tiny_vae import TinyDecoder


class UnfusedTinyDecoder(TinyDecoder):
    """the same network with a block as conv, conv, conv, add, ReLU: four round trips of the activation more than the fused kernel"""

    def _block(self, i, x, out):
        w, b = self.blocks[i]
        if getattr(self, "_tmp_shape", None) != x.shape:  # the two temporaries a fused block does not need, kept out of the timed region
            self._tmp, self._tmp_shape = (torch.empty_like(x), torch.empty_like(x)), x.shape
        t1, t2 = self._tmp
        ops.conv3x3_dense(x, w[0], b[0], t1, slope=0.0, act=True)
        ops.conv3x3_dense(t1, w[1], b[1], t2, slope=0.0, act=True)
        ops.conv3x3_dense(t2, w[2], b[2], t1)
        torch.add(t1, x, out=out).relu_()


def timed(rounds, kinds, reps=1):
    """kinds: {kind: callable}; -> {kind: [ms per call, one figure per round]}, kinds alternating inside a round; a round times `reps`
    back-to-back calls between one pair of events, so that a short kernel is not measured by its launch and the events"""
    ms = {k: [] for k in kinds}
    for _ in range(rounds):
        for k, call in kinds.items():
            call()  # untimed: warms this kind's code and buffers
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                call()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / reps)
    return ms


def report(tag, ms):
    for k, v in ms.items():
        print(json.dumps({"what": tag, "kind": k, "ms": [round(x, 4) for x in v], "median_ms": round(statistics.median(v), 4),
                          "spread_ms": round(max(v) - min(v), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kinds", default="vae,unfused,fused")
    ap.add_argument("--blocks", action="store_true", help="also time one residual block alone at 128^2 .. 1024^2")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tiny_ae_step: no GPU: there is nothing to time")
    dev = torch.device("cuda:0")
    h, w = args.height // 8, args.width // 8
    sd = synth.make_taef1_state_dict(seed=0)
    z = torch.randn(1, 16, h, w, generator=torch.Generator().manual_seed(0)).to(dev)
    kinds = {}
    with torch.inference_mode():
        if "vae" in args.kinds:
            import util

            cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
            from modules.autoencoder import AutoEncoder

            torch.manual_seed(0)
            ae = AutoEncoder(cfg.ae_params).to(dev).eval()

            def vae():
                with torch.autocast(device_type="cuda", dtype=torch.bfloat16, cache_enabled=False):
                    return ae.decode(z)

            kinds["vae"] = vae
        fused, unfused = TinyDecoder(sd, device=dev), UnfusedTinyDecoder(sd, device=dev)
        if "unfused" in args.kinds:
            kinds["unfused"] = lambda: unfused.decode_nhwc(z)
        if "fused" in args.kinds:
            kinds["fused"] = lambda: fused.decode_nhwc(z)
        if "unfused" in kinds and "fused" in kinds:  # faster and different is not faster: the two must agree to the blocks' rounding
            a, b = fused.decode_nhwc(z).float().clone(), unfused.decode_nhwc(z).float()
            print(json.dumps({"what": "fused vs unfused", "rel_l2": ((a - b).norm() / b.norm()).item()}), flush=True)
        report(f"decode {args.height}x{args.width}", timed(args.rounds, kinds))
        if args.blocks:
            wb, bb = fused.blocks[3]
            for n in (128, 256, 512, 1024):
                x = torch.randn(1, n, n, 64, device=dev).bfloat16()
                out = torch.empty_like(x)
                unfused_block = lambda: UnfusedTinyDecoder._block(fused, 3, x, out)
                report(f"block {n}x{n}, 50 back-to-back calls", timed(args.rounds, {"unfused": unfused_block, "fused": lambda: ops.conv3x3_block(x, wb, bb, out)}, reps=50))


if __name__ == "__main__":
    main()
