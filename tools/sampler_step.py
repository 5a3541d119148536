"""Time per EVALUATION of a frozen, graph-replayed denoise under a solver program (higher-order samplers) against the plain Euler one: full
Flux-dev geometry (19 + 38 blocks, hidden 3072) with synthetic weights made on the device, fp8 flow, a 1024^2 image (Li 4096, Lt 512), B 1.
One engine, five request kinds that ALTERNATE round after round in one process: plain Euler (today's kernels), ab2 (one evaluation per step),
heun (two per step but the last), heun + guided (true CFG: two samples in the engine), euler_ancestral (one evaluation per step, the noise
generated in the update kernel).  The meter is the engine's own hipEvent pair around the
graph replays (fluxmi_engine_last_timing), divided by the evaluations it brackets; calibration, the modulation table, the warm step and the
capture are outside it.  Printed per kind: every round's ms per evaluation, the median and the spread (max - min), and for the solver kinds
the distance from the plain median next to the plain kind's own spread.
    python tools/sampler_step.py [--steps 20] [--rounds 3] [--height 1024 --width 1024] [--scale 3.5]
Kernel times come from ONE separate run under the profiler (own process, no counters), summarised by this tool:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/sampler_step.py --rounds 1 --steps 10
    python tools/sampler_step.py --summarize DIR
which prints the update kernels (euler_kernel, solver_step_kernel plain, guided and with noise) side by side (calls, mean, the ratio to euler_kernel)
and the launch count per frozen evaluation of each kind (evaluations are delimited by advance_step_kernel; an evaluation's kind is its
update kernel), and fails unless a solver evaluation launches as many kernels as a plain step.
Prints one JSON line per measurement."""
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

SOLVER_KERNEL = re.compile(r"(?:^|[\s:])solver_step_kernel<\s*(\w+)\s*,\s*\w+\s*,\s*\w+\s*,\s*(\w+)\s*>")  # <CFG, PLAIN, BLEND, NOISE>
EULER_KERNEL = re.compile(r"(?:^|[\s:])euler_kernel<\s*(\w+)\s*,\s*\w+\s*,\s*(\w+)\s*>")  # <CFG, PLAIN, BLEND>


def update_kind(name):
    m = SOLVER_KERNEL.search(name)
    if m:
        return "solver" + (" + guided" if m.group(1) in ("true", "1") else "") + (" + noise" if m.group(2) in ("true", "1") else "")
    m = EULER_KERNEL.search(name)
    if m and m.group(1) not in ("true", "1") and m.group(2) not in ("true", "1"):
        return "plain"
    return None


def summarize(path):
    """per update kernel: calls / mean / ratio to euler_kernel; per kind: launches per GRAPH-REPLAYED evaluation (tools/inpaint_step.py's
    rule: calibrating evaluations, which launch set_timestep_kernel, are left out; the most frequent count of a kind is reported)"""
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
        k = update_kind(name)
        if k is not None:
            kind = k
            times.setdefault(k, []).append(e - s)
        calibrating = calibrating or "set_timestep_kernel" in name
        if "advance_step_kernel" in name:
            if kind is not None and not calibrating:
                steps.setdefault(kind, []).append(cur)
            cur, kind, calibrating = 0, None, False
    base = times.get("plain")
    base_mean = sum(base) / len(base) if base else None
    for k, t in times.items():
        mean = sum(t) / len(t)
        print(json.dumps(dict(what="update kernel, one profiler trace", kind=k, calls=len(t), mean_us=round(mean / 1e3, 3), min_us=round(min(t) / 1e3, 3),
                              max_us=round(max(t) / 1e3, 3), ratio_to_euler_kernel=round(mean / base_mean, 3) if base_mean else None)))
    per_step = {}
    for k, c in steps.items():
        mode = max(set(c), key=c.count)
        per_step[k] = mode
        print(json.dumps(dict(what="kernel launches per frozen evaluation (most frequent count among the kind's evaluations)", kind=k, evaluations=len(c),
                              launches=mode, evaluations_with_that_count=c.count(mode))))
    # the solver update REPLACES the update kernel: a solver evaluation must launch exactly what a plain step launches
    if "plain" in per_step and "solver" in per_step:
        same = per_step["plain"] == per_step["solver"]
        print(json.dumps(dict(what="solver evaluation launches as many kernels as the plain step", plain=per_step["plain"], solver=per_step["solver"],
                              equal=same)))
        if not same:
            sys.exit("the solver evaluation launches %d kernels, the plain step %d" % (per_step["solver"], per_step["plain"]))
    if "plain" in per_step and "solver + noise" in per_step:  # ... and so must one with noise: the generator adds no launch
        same = per_step["plain"] == per_step["solver + noise"]
        print(json.dumps(dict(what="solver evaluation with noise launches as many kernels as the plain step", plain=per_step["plain"],
                              noise=per_step["solver + noise"], equal=same)))
        if not same:
            sys.exit("the noise evaluation launches %d kernels, the plain step %d" % (per_step["solver + noise"], per_step["plain"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="user steps per request (heun: 2 * steps - 1 evaluations)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--scale", type=float, default=3.5)
    ap.add_argument("--summarize", default=None, help="a directory (or file) with a rocprofv3 *kernel_trace.csv of this tool: print the summary and exit")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    import torch

    import util
    from bench import util_schedule
    from float8_quantize import quantize_flow_transformer_and_dispatch_float8
    from fluxmi import _lib, solvers, synth

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
        neg = {k: v.to(dev) for k, v in synth.make_inputs(p, args.height, args.width, 512, batch=1, seed=100, real_tokens=8).items()}
        Li, Lt = inp["img"].shape[1], inp["txt"].shape[1]
        sched = lambda n: util_schedule(n, Li)  # noqa: E731

        def run(ts, sampler, guided):
            kw = dict(neg_txt=neg["txt"], neg_y=neg["y"], cfg_scale=args.scale) if guided else {}
            if sampler is not None:
                kw["solver"] = solvers.build_program(sampler, ts)
            if sampler in solvers.STOCHASTIC_SAMPLERS:
                kw["solver_noise"] = ([(1234, 0, 0, 0)], 0)
            return model.denoise(inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], ts, guidance=3.5, use_graph=True, **kw)

        run(sched(13), None, False)  # calibration: 13 unfused steps freeze every F8Linear input scale
        assert model.calibration_state()[0]
        kinds = (("plain", None, False), ("ab2", "ab2", False), ("heun", "heun", False), ("heun + guided", "heun", True),
                 ("euler_ancestral", "euler_ancestral", False))
        per = {name: [] for name, _, _ in kinds}
        evals = {}
        finite = True
        for _ in range(args.rounds):
            for name, sampler, guided in kinds:
                run(sched(2), sampler, guided)  # warm evaluation + capture (every switch of kind re-captures)
                out = run(sched(args.steps), sampler, guided)
                ms, n = _lib.C.c_float(0), _lib.C.c_int(0)
                _lib.call("fluxmi_engine_last_timing", model._engine, _lib.C.byref(ms), _lib.C.byref(n))
                per[name].append(ms.value / max(1, n.value))
                evals[name] = n.value
                finite = finite and bool(torch.isfinite(out.float()).all())
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        for name, sampler, guided in kinds:
            v = per[name]
            rec = dict(what="frozen graph-replayed Flux-dev evaluation (forward + update), kinds alternating in one process", kind=name, images=1,
                       engine_batch=2 if guided else 1, Li=Li, Lt=Lt, steps_per_request=args.steps, timed_evaluations=evals[name],
                       ms_per_evaluation_each_round=[round(t, 3) for t in v], ms_per_evaluation_median=round(med(v), 3),
                       spread_ms=round(max(v) - min(v), 3))
            if name in ("ab2", "heun", "euler_ancestral"):
                rec.update(minus_plain_median_ms=round(med(v) - med(per["plain"]), 3),
                           plain_spread_ms=round(max(per["plain"]) - min(per["plain"]), 3))
            print(json.dumps(rec), flush=True)
        print(json.dumps(dict(finite=finite)), flush=True)


if __name__ == "__main__":
    main()
