"""Time per step of a frozen, graph-replayed guided denoise WITH guidance shaping (CFG rescale, APG, CFG-Zero*; csrc/guidance.hip) against the
unshaped guided one: full Flux-dev geometry (19 + 38 blocks, hidden 3072) with synthetic weights made on the device, fp8 flow, a 1024^2 image
(Li 4096, Lt 512), one guided image (two samples in the engine).  One engine, one process, the request kinds ALTERNATING round after round,
so that drift of the device shows in every kind alike.  A shaped step is the unshaped step plus two launches (fluxmi_guidance_moments,
fluxmi_guidance_combine) in front of the update.  The meter is the engine's own hipEvent pair around the graph replays
(fluxmi_engine_last_timing); calibration, the modulation table, the warm step and the capture -- every switch between unshaped and shaped
re-captures, switches among shaped kinds do not -- are outside it.
    python tools/guidance_step.py [--steps 20] [--requests 5] [--height 1024 --width 1024] [--scale 3.5] [--kinds unshaped,rescale,apg,zero_star]
Prints one JSON line per kind: every request's ms per step, the median and the spread (max - min)."""
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
from fluxmi import _lib, synth

KINDS = {
    "unshaped": None,
    "rescale": dict(rescale=0.7),
    "apg": dict(mode="apg", eta=0.0, norm_threshold=15.0, momentum=-0.5),
    "zero_star": dict(mode="cfg_zero_star", zero_init_steps=1),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--requests", type=int, default=5)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--scale", type=float, default=3.5)
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
        neg = {k: v.to(dev) for k, v in synth.make_inputs(p, args.height, args.width, 512, batch=1, seed=100, real_tokens=8).items()}
        Li, Lt = inp["img"].shape[1], inp["txt"].shape[1]

        def run(n, kind):
            return model.denoise(inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], util_schedule(n, Li), guidance=3.5, use_graph=True,
                                 neg_txt=neg["txt"], neg_y=neg["y"], cfg_scale=args.scale, guidance_shaping=KINDS[kind])

        run(13, kinds[0])  # calibration: 13 unfused guided steps freeze every F8Linear input scale
        assert model.calibration_state()[0]
        per = {k: [] for k in kinds}
        finite = {k: True for k in kinds}
        for _ in range(args.requests):
            for k in kinds:
                out = run(args.steps, k)  # a switch of graph kind: warm step + capture in front of the timed replays
                ms, n = _lib.C.c_float(0), _lib.C.c_int(0)
                _lib.call("fluxmi_engine_last_timing", model._engine, _lib.C.byref(ms), _lib.C.byref(n))
                per[k].append(ms.value / max(1, n.value))
                finite[k] = finite[k] and bool(torch.isfinite(out.float()).all())
        for k in kinds:
            v = sorted(per[k])
            print(json.dumps(dict(what="frozen graph-replayed guided Flux-dev denoise step", kind=k, shaping=KINDS[k], images=1, engine_batch=2, Li=Li,
                                  Lt=Lt, steps_per_request=args.steps, ms_per_step_each=[round(x, 3) for x in per[k]],
                                  ms_per_step_median=round(v[len(v) // 2], 3), ms_per_step_spread=round(v[-1] - v[0], 3), finite=finite[k])),
                  flush=True)


if __name__ == "__main__":
    main()
