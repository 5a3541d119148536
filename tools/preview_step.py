"""Whole-request time of a frozen, graph-replayed Flux-dev denoise WITH progress / live previews (csrc/preview.hip; include/fluxmi.h,
fluxmi_engine_set_preview) against the plain request: full Flux-dev geometry (19 + 38 blocks, hidden 3072) with synthetic weights made on
the device, fp8 flow, a 1024^2 image (Li 4096, Lt 512), B = 1, 28 steps.  One engine, one process, the request kinds ALTERNATING round after
round, so that drift of the device shows in every kind alike:
    plain    no hook: today's request
    hook     a step hook with every = 0: progress and cancellation only -- the throttled loop (at most FLUXMI_PREVIEW_DEPTH evaluations
             ahead of the GPU, one event wait per evaluation) and no launch of its own
    every1   a preview at every evaluation: one more launch per step, one 393 KB device-to-host copy per delivery
    every4   a preview at every fourth evaluation: the same launches (the kernel returns at once on the others), a quarter of the copies
Two meters per request: the host's wall clock around the whole Flux.denoise call, stream-synchronised on both sides (what a caller waits
for; a hooked call is synchronous anyway), and the engine's own hipEvent pair around the graph replays (fluxmi_engine_last_timing).  Every
timed request follows an untimed one of its kind, which absorbs the warm step and the capture of a switch between previewed and not.
    python tools/preview_step.py [--steps 28] [--requests 5] [--height 1024 --width 1024] [--kinds plain,hook,every1,every4]
Prints one JSON line per kind: every request's ms, the median and the spread (max - min); "no cost" is judged against the plain kind's
own spread."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flux-fp8-api_amd"))
sys.path.insert(0, ROOT)
import torch

import util
from bench import util_schedule
from float8_quantize import quantize_flow_transformer_and_dispatch_float8
from fluxmi import _lib, synth
from modules.flux_model import PreviewCall

KINDS = {"plain": None, "hook": 0, "every1": 1, "every4": 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=28)
    ap.add_argument("--requests", type=int, default=5)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--kinds", default=",".join(KINDS), help="comma-separated, out of " + ", ".join(KINDS))
    args = ap.parse_args()
    kinds = [k for k in args.kinds.split(",") if k]
    for k in kinds:
        if k not in KINDS:
            ap.error(f"unknown kind {k!r}")
    dev = torch.device("cuda:0")
    with torch.inference_mode():
        cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16", quantize_modulation=True, quantize_flow_embedder_layers=False)
        p = cfg.params
        sd = synth.make_state_dict(p, seed=0, device=dev)
        model = util.load_flow_model(cfg, sd)
        del sd
        quantize_flow_transformer_and_dispatch_float8(model, dev, flow_dtype=torch.bfloat16, swap_linears_with_cublaslinear=False,
                                                      quantize_modulation=True, quantize_flow_embedder_layers=False)
        torch.cuda.empty_cache()
        inp = {k: v.to(dev) for k, v in synth.make_inputs(p, args.height, args.width, 512, batch=1, seed=0).items()}
        Li, Lt = inp["img"].shape[1], inp["txt"].shape[1]
        g = torch.Generator().manual_seed(0)
        proj = (0.1 * torch.randn(51, generator=g)).tolist()
        grid = (args.height // 16, args.width // 16)
        delivered = {k: 0 for k in kinds}

        def run(n, kind):
            every = KINDS[kind]
            pv = None
            if every is not None:
                def cb(evaluation, n_evaluations, rgb, kind=kind):
                    delivered[kind] += rgb is not None
                    return True

                pv = PreviewCall(proj if every else None, grid, every, 0, n, cb)
            return model.denoise(inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], util_schedule(n, Li), guidance=3.5, use_graph=True,
                                 preview=pv)

        run(13, "plain")  # calibration: 13 unfused steps freeze every F8Linear input scale
        assert model.calibration_state()[0]
        wall = {k: [] for k in kinds}
        per = {k: [] for k in kinds}
        outs = {}
        for _ in range(args.requests):
            for k in kinds:
                run(args.steps, k)  # untimed: the warm step and the capture of a switch of graph kind
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = run(args.steps, k)
                torch.cuda.synchronize()
                wall[k].append((time.perf_counter() - t0) * 1e3)
                ms, n = _lib.C.c_float(0), _lib.C.c_int(0)
                _lib.call("fluxmi_engine_last_timing", model._engine, _lib.C.byref(ms), _lib.C.byref(n))
                per[k].append(ms.value / max(1, n.value))
                outs.setdefault(k, out)
        for k in kinds:
            w, v = sorted(wall[k]), sorted(per[k])
            print(json.dumps(dict(what="whole frozen graph-replayed Flux-dev denoise request", kind=k, preview_every=KINDS[k],
                                  look_ahead=_lib.PREVIEW_DEPTH, images=1, Li=Li, Lt=Lt, steps=args.steps,
                                  request_ms_each=[round(x, 2) for x in wall[k]], request_ms_median=round(w[len(w) // 2], 2),
                                  request_ms_spread=round(w[-1] - w[0], 2), replay_ms_per_step_median=round(v[len(v) // 2], 3),
                                  replay_ms_per_step_spread=round(v[-1] - v[0], 3), previews_delivered=delivered[k],
                                  same_latents_as_first_kind=bool(torch.equal(outs[k], outs[kinds[0]])))), flush=True)


if __name__ == "__main__":
    main()
