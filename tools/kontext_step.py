"""Time per step of a frozen, graph-replayed FLUX.1 Kontext denoise: full Flux-dev geometry (19 + 38 blocks, hidden 3072) with synthetic
weights made on the device, fp8 flow, a 1024^2 image with a 1024^2 reference by default (L = 512 + 4096 + 4096 = 8704).  The meter is the
engine's own hipEvent pair around the graph replays (fluxmi_engine_last_timing); calibration, the modulation table and the capture are
outside it.  With --plain the same request without the reference (L = 4608), for comparison.
    python tools/kontext_step.py [--steps 20] [--requests 3] [--height 1024 --width 1024] [--ref 1024x1024] [--batch 1] [--plain]
Prints one JSON line."""
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
from flux_pipeline import kontext_reference_ids, kontext_reference_size
from float8_quantize import quantize_flow_transformer_and_dispatch_float8
from fluxmi import _lib, synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--requests", type=int, default=3)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--ref", default="1024x1024", help="reference image size WxH (snapped to Kontext's preferred resolutions)")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--plain", action="store_true", help="no reference: the txt2img request of the same size")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16", quantize_modulation=True, quantize_flow_embedder_layers=False)
    p = cfg.params
    with torch.inference_mode():
        sd = synth.make_state_dict(p, seed=0, device=dev)
        model = util.load_flow_model(cfg, sd)
        del sd
        quantize_flow_transformer_and_dispatch_float8(model, dev, flow_dtype=torch.bfloat16, swap_linears_with_cublaslinear=False,
                                                      quantize_modulation=True, quantize_flow_embedder_layers=False)
        torch.cuda.empty_cache()
        B = args.batch
        inp = {k: v.to(dev) for k, v in synth.make_inputs(p, args.height, args.width, 512, batch=B, seed=0).items()}
        Li, Lt = inp["img"].shape[1], inp["txt"].shape[1]
        cond = {}
        Lc = 0
        if not args.plain:
            rw, rh = (int(v) for v in args.ref.lower().split("x"))
            _, _, w_l, h_l = kontext_reference_size(rw, rh)
            Lc = (h_l // 2) * (w_l // 2)
            g = torch.Generator(device=dev).manual_seed(1)
            cond = dict(img_cond_seq=torch.randn(B, Lc, p.in_channels, generator=g, device=dev).to(torch.bfloat16),
                        img_cond_seq_ids=kontext_reference_ids(B, h_l, w_l, dev, torch.bfloat16))
        sched = lambda n: util_schedule(n, Li)  # noqa: E731  (the noisy tokens only)
        run = lambda ts, graph: model.denoise(inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], ts,  # noqa: E731
                                              guidance=3.5, use_graph=graph, **cond)
        run(sched(13), False)  # calibration: 13 unfused steps freeze every F8Linear input scale
        assert model.calibration_state()[0]
        run(sched(2), True)  # warm step + capture
        per = []
        for _ in range(args.requests):
            out = run(sched(args.steps), True)
            ms, n = _lib.C.c_float(0), _lib.C.c_int(0)
            _lib.call("fluxmi_engine_last_timing", model._engine, _lib.C.byref(ms), _lib.C.byref(n))
            per.append(ms.value / max(1, n.value))
        torch.cuda.synchronize()
        finite = bool(torch.isfinite(out.float()).all())
    per.sort()
    print(json.dumps(dict(what="frozen graph-replayed Flux-dev denoise step", kontext=not args.plain, B=B, Li=Li, Lc=Lc, Lt=Lt, L=Lt + Li + Lc,
                          steps_per_request=args.steps, ms_per_step_each=[round(v, 3) for v in per], ms_per_step_median=round(per[len(per) // 2], 3),
                          finite=finite)))


if __name__ == "__main__":
    main()
