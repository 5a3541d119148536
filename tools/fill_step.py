"""Time per step of a frozen, graph-replayed FLUX.1 Fill / Depth / Canny denoise against the plain one: full Flux-dev geometry (19 + 38
blocks, hidden 3072) with synthetic weights made on the device, fp8 flow, a 1024^2 image (Li 4096, Lt 512, B 1).  One engine per image-stream
width C_in -- 384 (Fill), 128 (Depth / Canny), 64 (text-to-image) -- built one after the other in this process; C_out is 64 for all three.
The meter is the engine's own hipEvent pair around the graph replays (fluxmi_engine_last_timing); calibration, the modulation table and the
capture are outside it.
    python tools/fill_step.py [--steps 20] [--requests 3] [--height 1024 --width 1024] [--batch 1] [--cin 384,128,64]
Prints one JSON line per C_in."""
import argparse
import gc
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


def one(c_in, args, dev):
    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16", quantize_modulation=True, quantize_flow_embedder_layers=False)
    p = cfg.params
    p.in_channels, p.out_channels = c_in, 64
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
    if c_in != 64:
        g = torch.Generator(device=dev).manual_seed(1)
        c = torch.randn(B, Li, c_in - 64, generator=g, device=dev)
        if c_in - 64 > 64:  # Fill: a binary mask behind the masked-image latents
            c[..., 64:] = (c[..., 64:] > 0.5).float()
        cond = dict(img_cond=c.to(torch.bfloat16))
    sched = lambda n: util_schedule(n, Li)  # noqa: E731
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
    model._invalidate_engine()
    del model, out, inp, cond
    gc.collect()
    torch.cuda.empty_cache()
    per.sort()
    kind = {384: "fill", 128: "depth/canny", 64: "plain"}.get(c_in, "other")
    return dict(what="frozen graph-replayed Flux-dev denoise step", kind=kind, C_in=c_in, C_out=64, B=B, Li=Li, Lt=Lt,
                steps_per_request=args.steps, ms_per_step_each=[round(v, 3) for v in per], ms_per_step_median=round(per[len(per) // 2], 3),
                finite=finite)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--requests", type=int, default=3)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--cin", default="384,128,64", help="image-stream widths to time, in this order")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    with torch.inference_mode():
        for c_in in (int(v) for v in args.cin.split(",")):
            print(json.dumps(one(c_in, args, dev)), flush=True)


if __name__ == "__main__":
    main()
