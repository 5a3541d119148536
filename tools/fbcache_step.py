"""What first-block step caching costs and saves: full Flux-dev geometry (19 + 38 blocks, hidden 3072) with synthetic weights made on the
device, fp8 flow, a 1024^2 image (Li 4096, Lt 512), B = 1, frozen and graph-replayed.  One engine:
  * ms per PLAIN step (the engine's hipEvent pair around the replays, fluxmi_engine_last_timing);
  * ms per ALL-MISS cached step (threshold 1e-30: head + host round trip + body every step) -- the price of the split and the extra passes;
  * ms per HIT step (threshold 1e30: every step behind the first is head + skip), from requests of two lengths so that the one miss cancels;
  * WALL-CLOCK of whole requests (--request-steps, 28) plain and cached with cache_max_hits 1, 2, 3 at threshold 1e30 (hit rate fixed by
    construction: 1/2, 2/3, 3/4 of the steps), next to misses x t_full + hits x t_hit.
Synthetic weights have no trained model's step-to-step smoothness: nothing here says how often a real model hits at a given threshold.
    python tools/fbcache_step.py [--steps 20] [--requests 3] [--height 1024 --width 1024] [--request-steps 28] [--only plain|miss|hit]
Prints one JSON line per measurement."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--requests", type=int, default=3)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--request-steps", type=int, default=28)
    ap.add_argument("--only", default=None, choices=("plain", "miss", "hit"), help="one kind of step only, twice (for a kernel trace)")
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
        inp = {k: v.to(dev) for k, v in synth.make_inputs(p, args.height, args.width, 512, batch=1, seed=0).items()}
        Li, Lt = inp["img"].shape[1], inp["txt"].shape[1]
        sched = lambda n: util_schedule(n, Li)  # noqa: E731

        def run(ts, **cache):
            return model.denoise(inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], ts, guidance=3.5, use_graph=True, **cache)

        def timed(ts, **cache):
            out = run(ts, **cache)
            ms, n = _lib.C.c_float(0), _lib.C.c_int(0)
            _lib.call("fluxmi_engine_last_timing", model._engine, _lib.C.byref(ms), _lib.C.byref(n))
            return ms.value, n.value, out

        run(sched(13))  # calibration: 13 unfused steps freeze every F8Linear input scale
        assert model.calibration_state()[0]
        kinds = {"plain": {}, "miss": dict(cache_threshold=1e-30), "hit": dict(cache_threshold=1e30)}
        if args.only:
            for _ in range(2):
                run(sched(args.steps), **kinds[args.only])
            torch.cuda.synchronize()
            print(json.dumps(dict(what="two requests of one kind (for a kernel trace)", kind=args.only, steps=args.steps,
                                  hits=sum(model.step_cache_log()[1]))), flush=True)
            return
        t = {}
        for name in ("plain", "miss"):
            run(sched(2), **kinds[name])  # warm step + capture
            per = []
            for _ in range(args.requests):
                ms, n, out = timed(sched(args.steps), **kinds[name])
                per.append(ms / max(1, n))
            assert name == "plain" or not any(model.step_cache_log()[1])
            per.sort()
            t[name] = per[len(per) // 2]
            print(json.dumps(dict(what="frozen graph-replayed Flux-dev denoise step", kind=name, Li=Li, Lt=Lt, steps_per_request=args.steps,
                                  ms_per_step_each=[round(v, 3) for v in per], ms_per_step_median=round(t[name], 3),
                                  finite=bool(torch.isfinite(out.float()).all()))), flush=True)
        print(json.dumps(dict(what="all-miss cached step over plain step", percent=round(100 * (t["miss"] / t["plain"] - 1), 2))), flush=True)
        # hit steps: a timed request of n steps is 1 miss + (n - 1) hits; two lengths cancel the miss
        run(sched(3), **kinds["hit"])
        per = []
        for _ in range(args.requests):
            ms_a, n_a, _ = timed(sched(args.steps), **kinds["hit"])
            ms_b, n_b, out = timed(sched(2 * args.steps), **kinds["hit"])
            assert sum(model.step_cache_log()[1]) == 2 * args.steps - 1
            per.append((ms_b - ms_a) / (n_b - n_a))
        per.sort()
        t["hit"] = per[len(per) // 2]
        print(json.dumps(dict(what="hit step (head + host decision + skip), from requests of two lengths", steps=[args.steps, 2 * args.steps],
                              ms_per_step_each=[round(v, 3) for v in per], ms_per_step_median=round(t["hit"], 3),
                              finite=bool(torch.isfinite(out.float()).all()))), flush=True)
        n = args.request_steps
        ts = sched(n)
        ref = None
        for max_hits in (0, 1, 2, 3):
            cache = dict(cache_threshold=1e30, cache_max_hits=max_hits) if max_hits else {}
            run(ts, **cache)
            wall = []
            for _ in range(args.requests):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = run(ts, **cache)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            wall.sort()
            hits = sum(model.step_cache_log()[1])
            ref = out if ref is None else ref
            rel = ((out.float() - ref.float()).norm() / ref.float().norm()).item()
            print(json.dumps(dict(what="wall-clock of one whole request", cache_max_hits=max_hits, steps=n, hits=hits, ms_each=[round(v, 1) for v in wall],
                                  ms_median=round(wall[len(wall) // 2], 1),
                                  model_ms=round((n - hits) * (t["miss"] if max_hits else t["plain"]) + hits * t["hit"], 1),
                                  rel_l2_vs_plain=round(rel, 4), finite=bool(torch.isfinite(out.float()).all()))), flush=True)


if __name__ == "__main__":
    main()
