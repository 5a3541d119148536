"""Time per step of a frozen, graph-replayed denoise with a FLUX ControlNet attached against the plain one: full Flux-dev geometry (19 + 38
blocks, hidden 3072) with synthetic weights made on the device, fp8 flow, a 1024^2 image (Li 4096, Lt 512), B 1.  One main engine, three request
kinds that ALTERNATE round after round in one process: plain, a 5 + 0 net (the small InstantX Canny / Depth shape), a 5 + 10 Union net (Lt + 1
text rows).  The meter is the engine's own hipEvent pair around the graph replays (fluxmi_engine_last_timing); calibration of all three
nets, the modulation tables, the warm step and the capture are outside it.  Printed per kind: every round's ms per step, the median, the
spread, the distance from the plain median, and the device bytes the engines own (fluxmi_engine_workspace_bytes) with and without a net.
Expectation (derived, not measured): the extra time is about the net's own blocks at the main blocks' per-block cost plus the adds.
    python tools/controlnet_step.py [--steps 20] [--rounds 3] [--height 1024 --width 1024]
Kernel times and launch counts come from ONE separate run under the profiler (own process, no counters), summarised by this tool:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/controlnet_step.py --rounds 1 --steps 6 --with-cache
    python tools/controlnet_step.py --summarize DIR
which prints add_scaled_kernel beside fb_resid_kernel (fluxmi_fb_apply, with --with-cache one step-cached request puts it into the trace;
the ControlNet's own x_embedder add uses it too): calls, mean time per launch and the GB/s on their 3 x n x 2 bytes, and the launches per
frozen step of each kind (steps are delimited by advance_step_kernel; a step's kind is its number of add_scaled launches; the steps of the
step-cached request, which carry fb_metric_kernel, are left out).
Prints one JSON line per measurement."""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flux-fp8-api_amd"))
sys.path.insert(0, ROOT)


def summarize(path, n_elems):
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True) if os.path.isdir(path) else [path]
    if not files:
        sys.exit("no *kernel_trace.csv under " + path)
    rows = []
    for f in files:
        rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))]
    rows.sort()
    times, steps, cur, adds, calibrating, cached = {}, {}, 0, 0, False, False
    for s, e, name in rows:
        cur += 1
        for key in ("add_scaled_kernel", "fb_resid_kernel<false"):
            if key in name:
                times.setdefault(key, []).append(e - s)
        adds += "add_scaled_kernel" in name
        calibrating = calibrating or "set_timestep_kernel" in name
        cached = cached or "fb_metric_kernel" in name  # a step of the --with-cache request: not a plain step
        if "advance_step_kernel" in name:
            if not calibrating and not cached:
                steps.setdefault(adds, []).append(cur)
            cur, adds, calibrating, cached = 0, 0, False, False
    for k, t in times.items():
        mean = sum(t) / len(t)
        print(json.dumps(dict(what="streaming add kernel, one profiler trace", kernel=k, calls=len(t), mean_us=round(mean / 1e3, 3),
                              min_us=round(min(t) / 1e3, 3), max_us=round(max(t) / 1e3, 3), bytes_per_launch=3 * n_elems * 2,
                              gb_per_s_at_mean=round(3 * n_elems * 2 / mean, 1))))
    for k, c in sorted(steps.items()):
        mode = max(set(c), key=c.count)
        print(json.dumps(dict(what="kernel launches per frozen step (most frequent count among the kind's steps)", add_scaled_launches_per_step=k,
                              steps=len(c), launches_per_step=mode, steps_with_that_count=c.count(mode))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--with-cache", action="store_true", help="one step-cached plain request at the end: puts fluxmi_fb_apply into a profiler trace")
    ap.add_argument("--summarize", default=None, help="a directory (or file) with a rocprofv3 *kernel_trace.csv of this tool: print the summary and exit")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize, (args.height // 16) * (args.width // 16) * 3072)
    import torch

    import util
    from bench import util_schedule
    from float8_quantize import quantize_flow_transformer_and_dispatch_float8
    from fluxmi import _lib, synth
    from modules.controlnet import ControlNetCall, FluxControlNet

    dev = torch.device("cuda:0")
    with torch.inference_mode():
        cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16", quantize_modulation=True, quantize_flow_embedder_layers=False)
        p = cfg.params
        q = dict(flow_dtype=torch.bfloat16, swap_linears_with_cublaslinear=False, quantize_modulation=True, quantize_flow_embedder_layers=False)
        sd = synth.make_state_dict(p, seed=0, device=dev)
        model = util.load_flow_model(cfg, sd)
        del sd
        quantize_flow_transformer_and_dispatch_float8(model, dev, **q)
        nets = {}
        for name, (nd, ns, nm) in (("net 5 + 0", (5, 0, 0)), ("net 5 + 10 (Union)", (5, 10, 7))):
            nsd = synth.make_controlnet_state_dict(p, nd, ns, nm, seed=1, device=dev)
            nets[name] = FluxControlNet.from_state_dict(cfg, nsd)
            del nsd
            quantize_flow_transformer_and_dispatch_float8(nets[name], dev, **q)
        torch.cuda.empty_cache()
        inp = {k: v.to(dev) for k, v in synth.make_inputs(p, args.height, args.width, 512, batch=1, seed=0).items()}
        Li, Lt = inp["img"].shape[1], inp["txt"].shape[1]
        cond = torch.randn(1, Li, 64, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).to(dev)
        sched = lambda n: util_schedule(n, Li)  # noqa: E731

        def run(ts, name, **kw):
            cn = None if name == "plain" else ControlNetCall(nets[name], cond, 0.7, 2 if nets[name].is_union else None)
            return model.denoise(inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], ts, guidance=3.5, use_graph=True, controlnet=cn, **kw)

        def owned(handle):
            b = _lib.C.c_longlong(0)
            _lib.call("fluxmi_engine_workspace_bytes", handle, _lib.C.byref(b))
            return b.value

        run(sched(13), "plain")  # calibration: 13 unfused steps freeze every F8Linear input scale of the main model ...
        for name in nets:
            run(sched(13), name)  # ... and of each net, on its own counter
        assert model.calibration_state()[0] and all(n.calibration_state()[0] for n in nets.values())
        kinds = ("plain",) + tuple(nets)
        per = {name: [] for name in kinds}
        finite = True
        for _ in range(args.rounds):
            for name in kinds:
                run(sched(2), name)  # warm step + capture (every switch of kind re-captures)
                out = run(sched(args.steps), name)
                ms, n = _lib.C.c_float(0), _lib.C.c_int(0)
                _lib.call("fluxmi_engine_last_timing", model._engine, _lib.C.byref(ms), _lib.C.byref(n))
                per[name].append(ms.value / max(1, n.value))
                finite = finite and bool(torch.isfinite(out.float()).all())
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        main_bytes = owned(model._engine)
        for name in kinds:
            v = per[name]
            net = nets.get(name)
            rec = dict(what="frozen graph-replayed Flux-dev denoise step, kinds alternating in one process", kind=name, Li=Li, Lt=Lt,
                       steps_per_request=args.steps, ms_per_step_each_round=[round(t, 3) for t in v], ms_per_step_median=round(med(v), 3),
                       spread_ms=round(max(v) - min(v), 3), minus_plain_median_ms=round(med(v) - med(per["plain"]), 3),
                       main_engine_bytes=main_bytes, net_engine_bytes=owned(net._engine) if net is not None else 0)
            if net is not None:
                nb, mb = net.params.depth + net.params.depth_single_blocks * 0.5, p.depth + p.depth_single_blocks * 0.5
                rec["derived_extra_ms_at_the_main_blocks_cost"] = round(med(per["plain"]) * nb / mb, 3)  # a single block ~ half a double block
            print(json.dumps(rec), flush=True)
        if args.with_cache:
            out = model.denoise(inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], sched(8), guidance=3.5, cache_threshold=1e9)
            finite = finite and bool(torch.isfinite(out.float()).all())
        print(json.dumps(dict(finite=finite)), flush=True)


if __name__ == "__main__":
    main()
