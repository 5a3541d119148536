"""Time per step of a frozen, graph-replayed GUIDED denoise (negative prompt, true classifier-free guidance) against the plain one: full
Flux-dev geometry (19 + 38 blocks, hidden 3072) with synthetic weights made on the device, fp8 flow, a 1024^2 image (Li 4096, Lt 512).  One
engine, three request kinds one after the other: plain B = 1, plain B = 2, guided B = 1 (two samples in the engine: the guided step is a
plain B = 2 step with another update kernel).  The meter is the engine's own hipEvent pair around the graph replays
(fluxmi_engine_last_timing); calibration, the modulation table and the capture are outside it.
With --interval lo,hi also the WALL-CLOCK of a whole request (--request-steps, 28) guided throughout, guided on the interval only, and plain:
the interval request is up to three denoise calls, and every switch between plain B = 1 and guided B = 1 re-allocates the workspace and
re-captures the step graph -- this is where that cost shows.
    python tools/cfg_step.py [--steps 20] [--requests 3] [--height 1024 --width 1024] [--scale 3.5] [--interval 0.0,0.5] [--request-steps 28]
Prints one JSON line per measurement."""
import argparse
import json
import math
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--requests", type=int, default=3)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--scale", type=float, default=3.5)
    ap.add_argument("--interval", default=None, help="lo,hi: also time whole requests guided on this fraction of the steps")
    ap.add_argument("--request-steps", type=int, default=28)
    args = ap.parse_args()
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
        inp = {k: v.to(dev) for k, v in synth.make_inputs(p, args.height, args.width, 512, batch=2, seed=0).items()}
        neg = {k: v.to(dev) for k, v in synth.make_inputs(p, args.height, args.width, 512, batch=2, seed=100, real_tokens=8).items()}
        Li, Lt = inp["img"].shape[1], inp["txt"].shape[1]
        sched = lambda n: util_schedule(n, Li)  # noqa: E731

        def run(ts, B, guided, img=None):
            kw = dict(neg_txt=neg["txt"][:B], neg_y=neg["y"][:B], cfg_scale=args.scale) if guided else {}
            return model.denoise(inp["img"][:B] if img is None else img, inp["img_ids"][:B], inp["txt"][:B], inp["txt_ids"][:B], inp["y"][:B], ts,
                                 guidance=3.5, use_graph=True, **kw)

        run(sched(13), 2, False)  # calibration: 13 unfused steps freeze every F8Linear input scale
        assert model.calibration_state()[0]
        for name, B, guided in (("plain", 1, False), ("plain", 2, False), ("guided", 1, True)):
            run(sched(2), B, guided)  # warm step + capture
            per = []
            for _ in range(args.requests):
                out = run(sched(args.steps), B, guided)
                ms, n = _lib.C.c_float(0), _lib.C.c_int(0)
                _lib.call("fluxmi_engine_last_timing", model._engine, _lib.C.byref(ms), _lib.C.byref(n))
                per.append(ms.value / max(1, n.value))
            per.sort()
            print(json.dumps(dict(what="frozen graph-replayed Flux-dev denoise step", kind=name, images=B, engine_batch=2 * B if guided else B,
                                  Li=Li, Lt=Lt, steps_per_request=args.steps, ms_per_step_each=[round(v, 3) for v in per],
                                  ms_per_step_median=round(per[len(per) // 2], 3), finite=bool(torch.isfinite(out.float()).all()))), flush=True)
        if args.interval:
            lo, hi = (float(v) for v in args.interval.split(","))
            n = args.request_steps
            ts = sched(n)
            g0, g1 = min(n, math.ceil(lo * n)), min(n, math.ceil(hi * n))  # FluxPipeline.generate's segments

            def request(kind):
                if kind == "plain":
                    return run(ts, 1, False)
                if kind == "guided":
                    return run(ts, 1, True)
                x = None
                for a, b, guided in ((0, g0, False), (g0, g1, True), (g1, n, False)):
                    if a < b:
                        x = run(ts[a:b + 1], 1, guided, img=x)
                return x

            for kind in ("plain", "guided", "interval"):
                wall = []
                for _ in range(args.requests):
                    request("guided" if kind == "plain" else "plain")  # every timed request starts from the OTHER kind's workspace and graph
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = request(kind)
                    torch.cuda.synchronize()
                    wall.append((time.perf_counter() - t0) * 1e3)
                wall.sort()
                print(json.dumps(dict(what="wall-clock of one whole request (after a request of another kind: one re-allocation + re-capture "
                                      "included; the interval request switches once more per boundary)", kind=kind, steps=n,
                                      guided_steps=(g1 - g0) if kind == "interval" else (n if kind == "guided" else 0),
                                      interval=[lo, hi] if kind == "interval" else None, ms_each=[round(v, 1) for v in wall],
                                      ms_median=round(wall[len(wall) // 2], 1), finite=bool(torch.isfinite(out.float()).all()))), flush=True)


if __name__ == "__main__":
    main()
