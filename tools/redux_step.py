"""FLUX.1 Redux costs on the GPU, one JSON line each:
  * a frozen, graph-replayed Flux-dev denoise step (19 + 38 blocks, hidden 3072, synthetic weights made on the device, fp8 flow, 1024^2,
    B 1) at text lengths Lt = 512 (plain), 1241 (512 T5 + 729 Redux tokens), 1242 and 1248.  1241 is odd, so the engine's row-pair
    activation layout is off there; 1242 keeps it and prices its loss; 1248 (a multiple of 16) also keeps the fused V^T and prices that.
    One engine, re-prepared per length; the meter is the engine's own hipEvent pair around the graph replays (fluxmi_engine_last_timing);
  * SigLIP-so400m + the Redux projector per image (random weights at the real geometry), hipEvent-timed, median of --reps after warm-up;
  * --switch: the cost of alternating plain and Redux requests on one engine (each switch re-prepares the workspace and re-captures).
Run it under `rocprofv3 --kernel-trace --stats -- python tools/redux_step.py --encoder-only` for the encoder's kernel split.
    python tools/redux_step.py [--steps 20] [--requests 3] [--lt 512,1241,1242,1248] [--reps 10] [--encoder-only] [--switch]"""
import argparse
import gc
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flux-fp8-api_amd"))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import util
from bench import util_schedule
from float8_quantize import quantize_flow_transformer_and_dispatch_float8
from fluxmi import _lib, synth


def flow_model(dev):
    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16", quantize_modulation=True, quantize_flow_embedder_layers=False)
    p = cfg.params
    sd = synth.make_state_dict(p, seed=0, device=dev)
    model = util.load_flow_model(cfg, sd)
    del sd
    quantize_flow_transformer_and_dispatch_float8(model, dev, flow_dtype=torch.bfloat16, swap_linears_with_cublaslinear=False,
                                                  quantize_modulation=True, quantize_flow_embedder_layers=False)
    torch.cuda.empty_cache()
    return model, p


def steps(args, dev):
    model, p = flow_model(dev)
    B = args.batch
    lts = [int(v) for v in args.lt.split(",")]
    inputs = {lt: {k: v.to(dev) for k, v in synth.make_inputs(p, args.height, args.width, lt, batch=B, seed=0, real_tokens=64).items()}
              for lt in lts}
    Li = inputs[lts[0]]["img"].shape[1]
    sched = lambda n: util_schedule(n, Li)  # noqa: E731

    def run(lt, ts, graph):
        d = inputs[lt]
        return model.denoise(d["img"], d["img_ids"], d["txt"], d["txt_ids"], d["y"], ts, guidance=3.5, use_graph=graph)

    def timed(lt):
        ms, n = _lib.C.c_float(0), _lib.C.c_int(0)
        out = run(lt, sched(args.steps), True)
        _lib.call("fluxmi_engine_last_timing", model._engine, _lib.C.byref(ms), _lib.C.byref(n))
        return out, ms.value / max(1, n.value)

    run(lts[0], sched(13), False)  # calibration at the first length: 13 unfused steps freeze every F8Linear input scale
    assert model.calibration_state()[0]
    for lt in lts:
        run(lt, sched(2), True)  # warm step + capture at this length
        per = []
        for _ in range(args.requests):
            out, v = timed(lt)
            per.append(v)
        torch.cuda.synchronize()
        per.sort()
        print(json.dumps(dict(what="frozen graph-replayed Flux-dev denoise step", B=B, Li=Li, Lt=lt, L=Li + lt, odd_Lt=lt % 2 == 1,
                              steps_per_request=args.steps, ms_per_step_each=[round(v, 3) for v in per],
                              ms_per_step_median=round(per[len(per) // 2], 3), finite=bool(torch.isfinite(out.float()).all()))), flush=True)
    if args.switch and len(lts) >= 2:
        # alternating requests: every change of Lt re-prepares the engine's workspace and re-captures its graph.  Overhead of a switch =
        # wall time of a request after the other length - wall time of the same request after one of its own length
        a, b = lts[0], lts[1]

        def wall(lt):
            t0 = time.perf_counter()
            run(lt, sched(args.steps), True)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        same = {a: [], b: []}
        switch = {a: [], b: []}
        for lt in (a, b):
            wall(lt)
            same[lt] += [wall(lt), wall(lt)]
        for i in range(4):
            lt = a if i % 2 == 0 else b  # the previous request had the other length
            switch[lt].append(wall(lt))
        over = {lt: round(float(np.median(switch[lt]) - np.median(same[lt])), 4) for lt in (a, b)}
        print(json.dumps(dict(what="alternating plain / Redux requests, wall time per request", Lt=[a, b], steps_per_request=args.steps,
                              s_same_shape={str(k): [round(v, 4) for v in vs] for k, vs in same.items()},
                              s_after_switch={str(k): [round(v, 4) for v in vs] for k, vs in switch.items()},
                              switch_overhead_s={str(k): v for k, v in over.items()})), flush=True)
    model._invalidate_engine()
    del model, inputs
    gc.collect()
    torch.cuda.empty_cache()


def encoder(args, dev):
    from modules.image_embedders import ReduxImageEncoder, SiglipVisionNative

    torch.manual_seed(0)
    with torch.device(dev), torch.no_grad():
        sig = SiglipVisionNative(None)  # google/siglip-so400m-patch14-384 geometry, default-initialised weights
        for name, t in sig.named_parameters():
            if t.dim() >= 2:
                t.copy_(torch.randn_like(t) / math.sqrt(t[0].numel()))
        enc = ReduxImageEncoder(sig)
        for lin in (enc.redux_up, enc.redux_down):
            lin.weight.copy_(torch.randn_like(lin.weight) / math.sqrt(lin.weight.shape[1]))
    enc = enc.to(dtype=torch.bfloat16)
    rng = np.random.default_rng(0)
    for n in (int(v) for v in args.images.split(",")):
        pix = torch.cat([enc.preprocess(rng.integers(0, 256, (512, 640, 3), dtype=np.uint8)) for _ in range(n)], 0).to(dev)

        def once():
            return enc.project(enc.siglip(pix)["last_hidden_state"])

        for _ in range(3):
            out = once()
        torch.cuda.synchronize()
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        enc_ms, proj_ms = [], []
        for _ in range(args.reps):
            e0.record()
            h = enc.siglip(pix)["last_hidden_state"]
            e1.record()
            out = enc.project(h)
            e2.record()
            e2.synchronize()
            enc_ms.append(e0.elapsed_time(e1))
            proj_ms.append(e1.elapsed_time(e2))
        tot = sorted(a + b for a, b in zip(enc_ms, proj_ms))
        print(json.dumps(dict(what="SigLIP-so400m + Redux projector (bf16, libfluxmi)", images=n, reps=args.reps,
                              siglip_ms_median=round(float(np.median(enc_ms)), 3), projector_ms_median=round(float(np.median(proj_ms)), 3),
                              total_ms_median=round(float(np.median(tot)), 3), ms_per_image=round(float(np.median(tot)) / n, 3),
                              out_shape=list(out.shape), finite=bool(torch.isfinite(out.float()).all()))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--requests", type=int, default=3)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--lt", default="512,1241,1242,1248", help="text lengths to time, in this order (the first one calibrates)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--images", default="1,2", help="images per encoder call")
    ap.add_argument("--encoder-only", action="store_true")
    ap.add_argument("--switch", action="store_true", help="also time alternating requests of the first two text lengths")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    encoder(args, dev)
    if not args.encoder_only:
        with torch.inference_mode():
            steps(args, dev)


if __name__ == "__main__":
    main()
