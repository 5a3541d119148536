"""Time per step of a frozen, graph-replayed FlowEdit evaluation (source_prompt: fluxmi.flowedit, Flux.denoise_edit) against the guided step
(negative prompt): full Flux-dev geometry (19 + 38 blocks, hidden 3072) with synthetic weights made on the device, fp8 flow, one 1024^2
image (Li 4096, Lt 512).  Both are ONE forward on two samples followed by one update launch -- euler_kernel's guided arm there, flowedit_kernel here --
so the edit step is expected inside the guided step's run-to-run spread.  One engine, the two request kinds ALTERNATING (--requests rounds)
so that clock and thermal drift hit both alike.  The meter is the engine's own hipEvent pair around the graph replays
(fluxmi_engine_last_timing); calibration, the modulation table and the capture are outside it.
    python tools/flowedit_step.py [--steps 20] [--requests 3] [--height 1024 --width 1024] [--n-avg 1] [--with-noise-sampler]
Prints one JSON line per kind.  --with-noise-sampler adds a third kind of the same engine shape, a guided `euler_ancestral` request, whose
update is the noise form of solver_step_kernel -- the other kernel that draws Philox normals -- for a kernel trace:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/flowedit_step.py --requests 1 --steps 6 --with-noise-sampler
    python tools/flowedit_step.py --summarize DIR"""
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
from fluxmi import _lib, flowedit, synth


UPDATE_KERNELS = (("flowedit", re.compile(r"flowedit_kernel<(?:true|1)>")), ("flowedit couple", re.compile(r"flowedit_kernel<(?:false|0)>")),
                  ("guided", re.compile(r"(?<![a-z_])euler_kernel<(?:true|1),\s*\w+,\s*(?:false|0)>")), ("guided solver + noise", re.compile(r"solver_step_kernel<(?:true|1),.*(?:true|1)>")))


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
                if k != "flowedit couple":
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--requests", type=int, default=3)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--n-avg", type=int, default=1)
    ap.add_argument("--with-noise-sampler", action="store_true", help="also a guided euler_ancestral request (the noise form of solver_step_kernel)")
    ap.add_argument("--summarize", default=None, help="a directory (or file) with a rocprofv3 *kernel_trace.csv of this tool: print the summary and exit")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
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
        other = {k: v.to(dev) for k, v in synth.make_inputs(p, args.height, args.width, 512, batch=1, seed=100, real_tokens=8).items()}
        Li, Lt = inp["img"].shape[1], inp["txt"].shape[1]
        sched = lambda n: util_schedule(n, Li)  # noqa: E731
        ids = flowedit.edit_ids(1234, 1)

        def guided(ts):
            return model.denoise(inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], ts, guidance=3.5, use_graph=True,
                                 neg_txt=other["txt"], neg_y=other["y"], cfg_scale=3.5)

        def edit(ts):
            return model.denoise_edit(inp["img"], inp["img_ids"], other["txt"], other["y"], inp["txt"], inp["y"], inp["txt_ids"], ts,
                                      n_avg=args.n_avg, ids=ids, source_guidance=1.5, guidance=5.5, use_graph=True)

        guided(sched(13))  # calibration: 13 unfused steps on the two-sample batch freeze every F8Linear input scale
        assert model.calibration_state()[0]
        def guided_noise(ts):
            from fluxmi import solvers

            prog = solvers.build_program("euler_ancestral", ts, 1.0, 1.0)
            return model.denoise(inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], ts, guidance=3.5, use_graph=True,
                                 neg_txt=other["txt"], neg_y=other["y"], cfg_scale=3.5, solver=prog, solver_noise=([(1234, 0, 0, 0)], 0))

        kinds = {"guided": guided, "flowedit": edit}
        if args.with_noise_sampler:
            kinds["guided euler_ancestral"] = guided_noise
        per = {k: [] for k in kinds}
        out = {}
        for k, run in kinds.items():
            run(sched(2))  # warm step + capture of this kind's graph (the two kinds never share one)
        for _ in range(args.requests):
            for k, run in kinds.items():
                out[k] = run(sched(args.steps))
                ms, n = _lib.C.c_float(0), _lib.C.c_int(0)
                _lib.call("fluxmi_engine_last_timing", model._engine, _lib.C.byref(ms), _lib.C.byref(n))
                per[k].append(ms.value / max(1, n.value))
        for k in kinds:
            v = sorted(per[k])
            print(json.dumps(dict(what="frozen graph-replayed Flux-dev step, one image = two samples in the engine", kind=k, Li=Li, Lt=Lt,
                                  evaluations_per_request=args.steps * (args.n_avg if k == "flowedit" else 1),
                                  ms_per_evaluation_each=[round(x, 3) for x in per[k]], ms_per_evaluation_median=round(v[len(v) // 2], 3),
                                  spread_ms=round(v[-1] - v[0], 3), finite=bool(torch.isfinite(out[k].float()).all()))), flush=True)


if __name__ == "__main__":
    main()
