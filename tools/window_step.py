"""Time per step of a frozen, graph-replayed WINDOWED evaluation (tile_size: fluxmi.windows, Flux.denoise_windows) against the plain step at
the same batch: full Flux-dev geometry (19 + 38 blocks, hidden 3072) with synthetic weights made on the device, fp8 flow, windows of 1024^2
(Li 4096, Lt 512), S windows of one canvas.  Both are ONE forward on S samples followed by one update launch -- euler_kernel there,
window_step_kernel here, which moves about 2 S MB -- so the windowed step is expected inside the plain step's run-to-run spread.  One
engine, the two request kinds ALTERNATING (--requests rounds) so that clock and thermal drift hit both alike.  The meter is the engine's own
hipEvent pair around the graph replays (fluxmi_engine_last_timing); calibration, the modulation table and the capture are outside it.
    python tools/window_step.py [--steps 10] [--requests 3] [--canvas 2048x1024] [--tile 1024] [--overlap 0] [--guided]
--canvas is width x height in pixels; 2048x1024 at overlap 0 gives S = 2, 2048x2048 at overlap 512 gives S = 9.  Prints one JSON line per
kind.  --guided adds the guided kinds (euler_kernel's guided arm against the guided windowed update, 2 S samples) for a kernel trace:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/window_step.py --requests 1 --steps 6 --guided
    python tools/window_step.py --summarize DIR"""
import argparse
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flux-fp8-api_amd"))
sys.path.insert(0, ROOT)
import torch

import util
from bench import util_schedule
from float8_quantize import quantize_flow_transformer_and_dispatch_float8
from fluxmi import _lib, synth, windows


UPDATE_KERNELS = (("windowed", re.compile(r"window_step_kernel<(?:true|1)>")), ("window gather", re.compile(r"window_step_kernel<(?:false|0)>")),
                  ("guided", re.compile(r"(?<![a-z_])euler_kernel<(?:true|1),\s*\w+,\s*(?:false|0)>")),
                  ("plain", re.compile(r"(?<![a-z_])euler_kernel<(?:false|0),\s*\w+,\s*(?:false|0)>")))  # <CFG, PLAIN, BLEND>


def summarize(path):
    """per update kernel of one rocprofv3 kernel trace: calls and mean duration; per kind: launches per GRAPH-REPLAYED evaluation (calibrating
    evaluations, which launch set_timestep_kernel, are left out; the most frequent count of a kind is reported)"""
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True) if os.path.isdir(path) else [path]
    if not files:
        sys.exit("no *kernel_trace.csv under " + path)
    rows = []
    for f in files:
        rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))]
    rows.sort()
    times, steps, cur, kind, calibrating = {}, {}, 0, None, False
    for s, e, name in rows:
        cur += 1
        for k, pat in UPDATE_KERNELS:
            if pat.search(name):
                times.setdefault(k, []).append(e - s)
                if k != "window gather":
                    kind = k
                break
        calibrating = calibrating or "set_timestep_kernel" in name
        if "advance_step_kernel" in name:
            if kind is not None and not calibrating:
                steps.setdefault(kind, []).append(cur)
            cur, kind, calibrating = 0, None, False
    for k, t in times.items():
        print(json.dumps(dict(what="update kernel, one profiler trace", kind=k, calls=len(t), mean_us=round(sum(t) / len(t) / 1e3, 3),
                              min_us=round(min(t) / 1e3, 3), max_us=round(max(t) / 1e3, 3))))
    for k, c in steps.items():
        mode = max(set(c), key=c.count)
        print(json.dumps(dict(what="kernel launches per frozen evaluation (most frequent count among the kind's evaluations)", kind=k,
                              evaluations=len(c), launches=mode, evaluations_with_that_count=c.count(mode))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--requests", type=int, default=3)
    ap.add_argument("--canvas", default="2048x1024", help="width x height of the canvas in pixels")
    ap.add_argument("--tile", type=int, default=1024)
    ap.add_argument("--overlap", type=int, default=0)
    ap.add_argument("--guided", action="store_true", help="also the guided kinds (2 S samples): euler_kernel's guided arm and the guided windowed update")
    ap.add_argument("--summarize", default=None, help="a directory (or file) with a rocprofv3 *kernel_trace.csv of this tool: print the summary and exit")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    width, height = (int(v) for v in args.canvas.lower().split("x"))
    t, stride = args.tile // 16, (args.tile - args.overlap) // 16
    plan = windows.plan(height // 16, width // 16, t, t, stride, stride, "cosine")
    S = plan.ny * plan.nx
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
        inp = {k: v.to(dev) for k, v in synth.make_inputs(p, args.tile, args.tile, 512, batch=1, seed=0).items()}
        other = {k: v.to(dev) for k, v in synth.make_inputs(p, args.tile, args.tile, 512, batch=1, seed=100, real_tokens=8).items()}
        Li, Lt = inp["img"].shape[1], inp["txt"].shape[1]
        sched = lambda n: util_schedule(n, Li)  # noqa: E731
        canvas = torch.randn(1, plan.Hc, plan.Wc, 64, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(dev)
        ex = lambda v, n: v.expand(n, *v.shape[1:]).contiguous()  # noqa: E731
        neg = dict(neg_txt=other["txt"], neg_y=other["y"], cfg_scale=3.5)

        def plain(ts, n=S, **kw):  # the plain (or guided) step at batch n: n stand-alone images of the window's size
            return model.denoise(ex(inp["img"], n), ex(inp["img_ids"], n), ex(inp["txt"], n), ex(inp["txt_ids"], n), ex(inp["y"], n), ts, guidance=3.5,
                                 use_graph=True, **kw)

        def windowed(ts, **kw):
            return model.denoise_windows(canvas, plan, inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], ts, guidance=3.5, use_graph=True, **kw)

        plain(sched(13))  # calibration: 13 unfused steps at batch S freeze every F8Linear input scale
        assert model.calibration_state()[0]
        kinds = {"plain": plain, "windowed": windowed}
        if args.guided:
            kinds["guided"] = lambda ts: plain(ts, **neg)
            kinds["guided windowed"] = lambda ts: windowed(ts, **neg)
        per = {k: [] for k in kinds}
        out = {}
        for _ in range(args.requests):
            for k, run in kinds.items():  # (kinds of one prepared shape never share a graph: every request warms and captures its own, untimed)
                out[k] = run(sched(args.steps))
                ms, n = _lib.C.c_float(0), _lib.C.c_int(0)
                _lib.call("fluxmi_engine_last_timing", model._engine, _lib.C.byref(ms), _lib.C.byref(n))
                per[k].append(ms.value / max(1, n.value))
        for k in kinds:
            v = sorted(per[k])
            print(json.dumps(dict(what="frozen graph-replayed Flux-dev step", kind=k, canvas=f"{width}x{height}", tile=args.tile, overlap=args.overlap,
                                  samples=S * (2 if "guided" in k else 1), Li=Li, Lt=Lt, evaluations_per_request=args.steps,
                                  ms_per_evaluation_each=[round(x, 3) for x in per[k]], ms_per_evaluation_median=round(v[len(v) // 2], 3),
                                  spread_ms=round(v[-1] - v[0], 3), finite=bool(torch.isfinite(out[k].float()).all()))), flush=True)


if __name__ == "__main__":
    main()
