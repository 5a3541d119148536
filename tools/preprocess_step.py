"""The control-map preprocessors (csrc/preprocess.hip) at a request's size: hysteresis round counts, per-call times and the whole
FluxPipeline.preprocess_control(photo, "canny") beside the numpy reference of tests/preprocess_ref.py on the same host.
    python tools/preprocess_step.py [--size 1024] [--reps 20]
Two synthetic inputs: "photo" (smooth ramps, discs and bars under mild noise: long thin edges) and "noise" (uniform noise: dense edges).
Times are hipEvent pairs around `reps` back-to-back calls (classify, one hysteresis round, gray, blur) or a host clock around calls that
end in their own synchronise (canny, preprocess_control).  Prints one JSON line per figure.  For the kernels' own durations:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/preprocess_step.py --reps 3 --no-reference"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "flux-fp8-api_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)
import numpy as np
import torch


def photo_like(n, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:n, 0:n]
    img = np.stack([xx, yy, (xx + yy) / 2], -1) * (160.0 / n) + 20
    for _ in range(40):
        cy, cx, rad = rng.uniform(0, n), rng.uniform(0, n), rng.uniform(n / 60, n / 6)
        img[(yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad] += rng.uniform(-70, 70, 3)
    for _ in range(12):
        a, w = int(rng.integers(0, n)), int(rng.integers(2, n // 20))
        img[:, a:a + w] += rng.uniform(-40, 40, 3)
        img[a:a + w // 2 + 1] += rng.uniform(-25, 25, 3)
    return np.clip(np.rint(img + rng.normal(0, 2.0, img.shape)), 0, 255).astype(np.uint8)


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def wall_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(float(np.median(t)), 3), min_ms=round(min(t), 3), max_ms=round(max(t), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-reference", action="store_true", help="skip the numpy reference and the equality check")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("preprocess_step: needs the GPU")
    from flux_pipeline import FluxPipeline
    from fluxmi import ops

    dev, n = torch.device("cuda:0"), a.size
    say = lambda **kw: print(json.dumps(kw), flush=True)
    inputs = {"photo": photo_like(n), "noise": np.random.default_rng(1).integers(0, 256, (n, n, 3), dtype=np.uint8)}
    pipe = FluxPipeline.__new__(FluxPipeline)
    pipe.ae, pipe.device_ae, pipe.device_flux = None, dev, dev
    for name, img in inputs.items():
        x = torch.from_numpy(img).to(dev)[None]
        edges, rounds = ops.canny(x, 100, 200, return_rounds=True)
        state = ops.canny_classify(x, 100, 200)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        say(what="canny", input=name, size=n, low=100, high=200, rounds=rounds, weak=int((state == 1).sum()), strong=int((state == 2).sum()),
            edge_pixels=int((edges == 255).sum()))
        say(what="canny_classify", input=name, size=n, ms=round(event_ms(lambda: ops.canny_classify(x, 100, 200, out=state), a.reps), 4),
            bytes=4 * n * n)
        st = state.clone()
        one = lambda: ops.call("fluxmi_canny_hysteresis_round", ops._p(st), n, n * n, 1, n, n, ops._p(flag), ops._stream())
        say(what="one hysteresis round (first: on the classify map; then at its fixed point)", input=name, size=n,
            first_ms=round(event_ms(lambda: (st.copy_(state), one()), 1) , 4), fixed_point_ms=round(event_ms(one, a.reps), 4))
        say(what="canny (classify + rounds + read-backs, host clock)", input=name, size=n, **wall_ms(lambda: ops.canny(x, 100, 200), a.reps))
        if name == "photo":
            g = torch.empty(1, n, n, dtype=torch.uint8, device=dev)
            say(what="rgb_to_gray", size=n, ms=round(event_ms(lambda: ops.rgb_to_gray(x, out=g), a.reps), 4), bytes=4 * n * n)
            b = torch.empty_like(x)
            say(what="gaussian_blur sigma 8 (radius 24), C 3, work buffer allocated per call", size=n,
                ms=round(event_ms(lambda: ops.gaussian_blur(x, 8.0, out=b), a.reps), 4))
            say(what="preprocess_control(photo, 'canny'), host array in, host uint8 [H, W, 3] out", size=n,
                **wall_ms(lambda: pipe.preprocess_control(img, "canny"), max(3, a.reps // 4)))
        if not a.no_reference:
            import preprocess_ref as pr

            t0 = time.perf_counter()
            want = pr.canny(img, 100, 200)
            say(what="numpy reference canny (tests/preprocess_ref.py), same host", input=name, size=n, ms=round((time.perf_counter() - t0) * 1e3, 1),
                equal=bool(np.array_equal(edges.cpu().numpy()[0], want)))


if __name__ == "__main__":
    main()
