"""Time per step of a frozen, graph-replayed REGIONAL denoise (token-group attention mask) against the dense one at the same text length:
full Flux-dev geometry (19 + 38 blocks, hidden 3072) with synthetic weights made on the device, fp8 flow, a 1024^2 image (Li 4096) and a text
stream of 512 base rows + 2 x 128 region rows (Lt 768, L 4864).  The table is flux_pipeline.build_region_groups on two boxes (left 55 %, right
55 %: they overlap in the middle).  One engine, the dense request first, then the masked one (masked versus dense is a graph kind: the switch
re-captures, outside the meter).  The meter is the engine's own hipEvent pair around the graph replays (fluxmi_engine_last_timing).
    python tools/regional_step.py [--steps 20] [--requests 3] [--height 1024 --width 1024] [--regional-tokens 128]
Prints one JSON line per measurement.  Under `rocprofv3 --kernel-trace --stats -- python tools/regional_step.py --requests 1` the masked and
the dense attention launches are two kernel names (the MASKED instantiation carries one more template argument)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flux-fp8-api_amd"))
sys.path.insert(0, ROOT)
import torch

import util
from bench import util_schedule
from float8_quantize import quantize_flow_transformer_and_dispatch_float8
from flux_pipeline import build_region_groups, region_token_grid
from fluxmi import _lib, synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--requests", type=int, default=3)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--regional-tokens", type=int, default=128)
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
        n_base, rt = 512, args.regional_tokens
        inp = {k: v.to(dev) for k, v in synth.make_inputs(p, args.height, args.width, n_base + 2 * rt, batch=1, seed=0).items()}
        Li, Lt = inp["img"].shape[1], inp["txt"].shape[1]
        grids = torch.stack([region_token_grid({"prompt": "", "box": b}, args.height, args.width) for b in ((0.0, 0.0, 0.55, 1.0), (0.45, 0.0, 1.0, 1.0))])
        table = build_region_groups(n_base, rt, grids)[None].to(dev)
        sched = lambda n: util_schedule(n, Li)  # noqa: E731

        def run(ts, masked):
            return model.denoise(inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], ts, guidance=3.5, use_graph=True,
                                 attn_groups=table if masked else None)

        run(sched(13), False)  # calibration: 13 unfused steps freeze every F8Linear input scale
        assert model.calibration_state()[0]
        for name, masked in (("dense", False), ("masked", True)):
            run(sched(2), masked)  # warm step + capture
            per = []
            for _ in range(args.requests):
                out = run(sched(args.steps), masked)
                ms, n = _lib.C.c_float(0), _lib.C.c_int(0)
                _lib.call("fluxmi_engine_last_timing", model._engine, _lib.C.byref(ms), _lib.C.byref(n))
                per.append(ms.value / max(1, n.value))
            per.sort()
            print(json.dumps(dict(what="frozen graph-replayed Flux-dev denoise step", kind=name, Li=Li, Lt=Lt, regional_tokens=rt,
                                  steps_per_request=args.steps, ms_per_step_each=[round(v, 3) for v in per],
                                  ms_per_step_median=round(per[len(per) // 2], 3), finite=bool(torch.isfinite(out.float()).all()))), flush=True)


if __name__ == "__main__":
    main()
