"""Time per step of a frozen, graph-replayed MASKED denoise (latent-blend inpainting) against the plain one: full Flux-dev geometry (19 + 38
blocks, hidden 3072) with synthetic weights made on the device, fp8 flow, a 1024^2 image (Li 4096, Lt 512), B 1.  One engine, three request
kinds that ALTERNATE round after round in one process: plain, masked, masked + guided (true CFG: two samples in the engine).  The meter is the
engine's own hipEvent pair around the graph replays (fluxmi_engine_last_timing); calibration, the modulation table, the warm step and the
capture are outside it.  Printed per kind: every round's ms per step, the median and the spread (max - min), and for the masked kind its
distance from the plain median next to the plain kind's own spread.
    python tools/inpaint_step.py [--steps 20] [--rounds 3] [--height 1024 --width 1024] [--scale 3.5] [--differential]
Kernel times come from ONE separate run under the profiler (own process, no counters), summarised by this tool:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/inpaint_step.py --rounds 1 --steps 10 --with-guided
    python tools/inpaint_step.py --summarize DIR
which prints the arms of euler_kernel<CFG, PLAIN, BLEND> (plain, guided, masked, masked + guided) side by side (calls, mean, the ratio to the plain arm) and the launch count per frozen step of each
kind (steps are delimited by advance_step_kernel; a step's kind is its update kernel), and fails unless a masked step launches as many
kernels as a plain one.
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

EULER_KERNEL = re.compile(r"(?:^|[\s:])euler_kernel<\s*(\w+)\s*,\s*\w+\s*,\s*(\w+)\s*>")  # <CFG, PLAIN, BLEND>
UPDATE_KERNELS = {(False, False): "plain", (True, False): "guided (no mask)", (False, True): "masked", (True, True): "masked + guided"}


def update_kind(name):
    m = EULER_KERNEL.search(name)
    return UPDATE_KERNELS[(m.group(1) in ("true", "1"), m.group(2) in ("true", "1"))] if m else None


def summarize(path):
    """per update kernel: calls / mean / ratio to euler_kernel; per step kind: launches per GRAPH-REPLAYED step.  A replayed step has no
    set_timestep_kernel (the calibrating steps do: they are left out) and is not the eager warm step in front of a capture, nor the step
    that follows a modulation-table build; those differ in their launch count from the kind's most frequent one, which is reported with
    how many steps had it."""
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
        print(json.dumps(dict(what="kernel launches per frozen step (most frequent count among the kind's steps)", kind=k, steps=len(c),
                              launches_per_step=mode, steps_with_that_count=c.count(mode))))
    # the blend REPLACES the update kernel: a masked step must launch exactly what a plain step launches
    if "plain" in per_step and "masked" in per_step:
        same = per_step["plain"] == per_step["masked"]
        print(json.dumps(dict(what="masked step launches as many kernels as the plain step", plain=per_step["plain"], masked=per_step["masked"], equal=same)))
        if not same:
            sys.exit("the masked step launches %d kernels, the plain step %d" % (per_step["masked"], per_step["plain"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--scale", type=float, default=3.5)
    ap.add_argument("--differential", action="store_true", help="the masked kinds run the differential form (a threshold per step)")
    ap.add_argument("--with-guided", action="store_true", help="a fourth kind, guided without a mask: puts the guided arm of euler_kernel into a profiler trace")
    ap.add_argument("--summarize", default=None, help="a directory (or file) with a rocprofv3 *kernel_trace.csv of this tool: print the summary and exit")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    import torch

    import util
    from bench import util_schedule
    from float8_quantize import quantize_flow_transformer_and_dispatch_float8
    from fluxmi import _lib, synth

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
        g = torch.Generator().manual_seed(5)
        x0, noise = (torch.randn(1, Li, 64, generator=g).to(torch.bfloat16).to(dev) for _ in range(2))
        mask = torch.zeros(1, args.height // 16, args.width // 16, 64)
        mask[:, args.height // 64:3 * args.height // 64, args.width // 64:3 * args.width // 64] = 1.0  # the centre quarter is regenerated
        mask = mask.reshape(1, Li, 64).to(torch.bfloat16).to(dev)
        if args.differential:
            mask = (mask * torch.rand(1, Li, 64, generator=g).to(dev)).to(torch.bfloat16)
        sched = lambda n: util_schedule(n, Li)  # noqa: E731

        def run(ts, masked, guided):
            kw = dict(neg_txt=neg["txt"], neg_y=neg["y"], cfg_scale=args.scale) if guided else {}
            if masked:
                kw.update(inpaint_x0=x0, inpaint_noise=noise, inpaint_mask=mask)
                if args.differential:
                    n = len(ts) - 1
                    kw.update(inpaint_thresholds=[1.0 - (i + 1) / n for i in range(n)])
            return model.denoise(inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], ts, guidance=3.5, use_graph=True, **kw)

        run(sched(13), False, False)  # calibration: 13 unfused steps freeze every F8Linear input scale
        assert model.calibration_state()[0]
        kinds = (("plain", False, False), ("masked", True, False), ("masked + guided", True, True))
        if args.with_guided:
            kinds += (("guided (no mask)", False, True),)
        per = {name: [] for name, _, _ in kinds}
        finite = True
        for _ in range(args.rounds):
            for name, masked, guided in kinds:
                run(sched(2), masked, guided)  # warm step + capture (every switch of kind re-captures)
                out = run(sched(args.steps), masked, guided)
                ms, n = _lib.C.c_float(0), _lib.C.c_int(0)
                _lib.call("fluxmi_engine_last_timing", model._engine, _lib.C.byref(ms), _lib.C.byref(n))
                per[name].append(ms.value / max(1, n.value))
                finite = finite and bool(torch.isfinite(out.float()).all())
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        for name, masked, guided in kinds:
            v = per[name]
            rec = dict(what="frozen graph-replayed Flux-dev denoise step, kinds alternating in one process", kind=name, images=1,
                       engine_batch=2 if guided else 1, differential=bool(args.differential and masked), Li=Li, Lt=Lt, steps_per_request=args.steps,
                       ms_per_step_each_round=[round(t, 3) for t in v], ms_per_step_median=round(med(v), 3), spread_ms=round(max(v) - min(v), 3))
            if name == "masked":
                rec.update(minus_plain_median_ms=round(med(v) - med(per["plain"]), 3),
                           plain_spread_ms=round(max(per["plain"]) - min(per["plain"]), 3))
            print(json.dumps(rec), flush=True)
        print(json.dumps(dict(finite=finite)), flush=True)


if __name__ == "__main__":
    main()
