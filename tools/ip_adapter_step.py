"""Time per step of a frozen, graph-replayed denoise with a FLUX IP-Adapter against the plain one: full Flux-dev geometry (19 + 38 blocks,
hidden 3072) with synthetic weights made on the device, fp8 flow, a 1024^2 image (Li 4096, Lt 512), B 1.  One engine, two request kinds that
ALTERNATE round after round in one process: plain, and an adapter of T tokens (default 4: XLabs v1) whose K / V are random device tensors
(the kernel's time does not depend on their values).  The meter is the engine's own hipEvent pair around the graph replays
(fluxmi_engine_last_timing); calibration, the modulation table, the warm step and the capture are outside it.  Printed per kind: every
round's ms per step, the median, the spread, the distance from the plain median and the device bytes the engine owns.
Expectation (derived, not measured): the extra time is 19 launches that each move what add_scaled_kernel moves on the image rows.
    python tools/ip_adapter_step.py [--steps 20] [--rounds 3] [--tokens 4] [--height 1024 --width 1024]
Kernel times and launch counts come from ONE separate run under the profiler (own process, no counters), summarised by this tool:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ip_adapter_step.py --rounds 1 --steps 6 --with-add-scaled
    python tools/ip_adapter_step.py --summarize DIR
which prints ip_attention_kernel beside add_scaled_kernel FROM THE SAME TRACE (--with-add-scaled launches fluxmi_add_scaled on the engine's
own image rows, as often as the adapter kernel ran: same bytes, same buffers): calls, mean time per launch, and the launches per frozen step
of each kind (steps are delimited by advance_step_kernel; a step's kind is its number of ip_attention launches).
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
    times, steps, cur, ips, calibrating = {}, {}, 0, 0, False
    for s, e, name in rows:
        cur += 1
        for key in ("ip_attention_kernel<true", "add_scaled_kernel"):
            if key in name:
                times.setdefault(key, []).append(e - s)
        ips += "ip_attention_kernel" in name
        calibrating = calibrating or "set_timestep_kernel" in name
        if "advance_step_kernel" in name:
            if not calibrating:
                steps.setdefault(ips, []).append(cur)
            cur, ips, calibrating = 0, 0, False
    for k, t in times.items():
        mean = sum(t) / len(t)
        print(json.dumps(dict(what="per-block streaming kernels on the image rows, one profiler trace", kernel=k, calls=len(t),
                              mean_us=round(mean / 1e3, 3), min_us=round(min(t) / 1e3, 3), max_us=round(max(t) / 1e3, 3),
                              bytes_per_launch=3 * n_elems * 2, gb_per_s_at_mean=round(3 * n_elems * 2 / mean, 1))))
    if len(times) == 2:
        a, b = (sum(times[k]) / len(times[k]) for k in ("ip_attention_kernel<true", "add_scaled_kernel"))
        print(json.dumps(dict(what="ip_attention_kernel / add_scaled_kernel, mean time per launch, same trace (expectation <= 1.5)", ratio=round(a / b, 3))))
    for k, c in sorted(steps.items()):
        mode = max(set(c), key=c.count)
        print(json.dumps(dict(what="kernel launches per frozen step (most frequent count among the kind's steps)", ip_attention_launches_per_step=k,
                              steps=len(c), launches_per_step=mode, steps_with_that_count=c.count(mode))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=4)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--with-add-scaled", action="store_true", help="launch fluxmi_add_scaled on the engine's image rows at the end: puts add_scaled_kernel into a profiler trace")
    ap.add_argument("--summarize", default=None, help="a directory (or file) with a rocprofv3 *kernel_trace.csv of this tool: print the summary and exit")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize, (args.height // 16) * (args.width // 16) * 3072)
    import torch

    import util
    from bench import util_schedule
    from float8_quantize import quantize_flow_transformer_and_dispatch_float8
    from fluxmi import _lib, ops, synth
    from modules.ip_adapter import IPAdapterCall

    dev = torch.device("cuda:0")
    with torch.inference_mode():
        cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16", quantize_modulation=True, quantize_flow_embedder_layers=False)
        p = cfg.params
        q = dict(flow_dtype=torch.bfloat16, swap_linears_with_cublaslinear=False, quantize_modulation=True, quantize_flow_embedder_layers=False)
        sd = synth.make_state_dict(p, seed=0, device=dev)
        model = util.load_flow_model(cfg, sd)
        del sd
        quantize_flow_transformer_and_dispatch_float8(model, dev, **q)
        torch.cuda.empty_cache()
        inp = {k: v.to(dev) for k, v in synth.make_inputs(p, args.height, args.width, 512, batch=1, seed=0).items()}
        Li, Lt = inp["img"].shape[1], inp["txt"].shape[1]
        g = torch.Generator(device=dev).manual_seed(5)
        kv = [torch.randn(p.depth, 1, args.tokens, p.hidden_size, generator=g, device=dev).to(torch.bfloat16) for _ in range(2)]
        call = IPAdapterCall(kv[0], kv[1], 0.7)
        sched = lambda n: util_schedule(n, Li)  # noqa: E731

        def run(ts, name):
            return model.denoise(inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], ts, guidance=3.5, use_graph=True,
                                 ip_adapter=None if name == "plain" else call)

        def owned():
            b = _lib.C.c_longlong(0)
            _lib.call("fluxmi_engine_workspace_bytes", model._engine, _lib.C.byref(b))
            return b.value

        run(sched(13), "plain")  # calibration: 13 unfused steps freeze every F8Linear input scale
        assert model.calibration_state()[0]
        kinds = ("plain", f"ip-adapter T {args.tokens}")
        per, bytes_ = {name: [] for name in kinds}, {}
        finite = True
        for _ in range(args.rounds):
            for name in kinds:
                run(sched(2), name)  # warm step + capture (every switch of kind re-captures)
                out = run(sched(args.steps), name)
                ms, n = _lib.C.c_float(0), _lib.C.c_int(0)
                _lib.call("fluxmi_engine_last_timing", model._engine, _lib.C.byref(ms), _lib.C.byref(n))
                per[name].append(ms.value / max(1, n.value))
                bytes_[name] = owned()
                finite = finite and bool(torch.isfinite(out.float()).all())
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        for name in kinds:
            v = per[name]
            print(json.dumps(dict(what="frozen graph-replayed Flux-dev denoise step, kinds alternating in one process", kind=name, Li=Li, Lt=Lt,
                                  steps_per_request=args.steps, ms_per_step_each_round=[round(t, 3) for t in v], ms_per_step_median=round(med(v), 3),
                                  spread_ms=round(max(v) - min(v), 3), minus_plain_median_ms=round(med(v) - med(per["plain"]), 3),
                                  engine_bytes=bytes_[name])), flush=True)
        if args.with_add_scaled:  # the ControlNet hand-over kernel on the same rows of the same buffer, for the profiler trace
            x, nb = _lib.C.c_void_p(), _lib.C.c_longlong(0)
            _lib.call("fluxmi_engine_get_buffer", model._engine, b"x", _lib.C.byref(x), _lib.C.byref(nb))
            H = p.hidden_size
            r = torch.randn(Li * H, generator=g, device=dev).to(torch.bfloat16)
            s = torch.full((1,), 0.7, dtype=torch.float32, device=dev)
            for _ in range(p.depth * args.steps):
                _lib.call("fluxmi_add_scaled", _lib.C.c_void_p(x.value + Lt * H * 2), (Lt + Li) * H, ops._p(r), Li * H, ops._p(s), 1, Li * H, ops._stream())
            torch.cuda.synchronize()
        print(json.dumps(dict(finite=finite)), flush=True)


if __name__ == "__main__":
    main()
