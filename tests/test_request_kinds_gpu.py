"""Every kind of denoise request in turn on ONE engine and ONE prepared shape (six samples of 16 image rows and 64 text rows): what a captured
step graph bakes in is one key (csrc/engine_state.h, StepKey), so a request that follows another kind captures its own pieces, an immediate
repeat replays them, and every result equals the kind's own first result and its eager (use_graph=False) result bit for bit.  The capture
counts after each visit and the bytes the engine owns after the whole sequence are RECORDED values (profiles/request_kinds.txt, taken from
the engine before its request state was gathered into one descriptor, one key and one side-buffer helper): a lost or resized allocation or
another re-capture decision changes them.  Requests are built by the feature tests' own helpers."""
import ctypes as C
import os

import pytest
import torch

import flux_oracle as fo
import inpaint_util as iu
import test_inpaint_gpu as t_inp
import test_preview_gpu as t_pv
import test_regional_gpu as t_reg
import test_solvers_gpu as t_sol
import test_stochastic_gpu as t_sto
from test_cfg_gpu import QUANTS, build, guided_denoise, plain_denoise, rel_l2, tiny_config, to_dev
from test_flowedit_gpu import captures, run_edit
from test_guidance_gpu import SHAPINGS, shaped_denoise
from test_windows_gpu import HC, WC, make_plan, run_windows

pytestmark = pytest.mark.gpu

RECORD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "request_kinds.txt")


def recorded():
    vals = {}
    with open(RECORD) as f:
        for line in f:
            if ":" in line and not line.startswith("#"):
                k, v = line.split(":", 1)
                vals[k.strip()] = [int(x) for x in v.split()]
    return vals["captures"], vals["workspace_bytes"][0]


def test_request_kinds_in_turn(dev):
    from fluxmi import _lib

    cfg = tiny_config()
    model, _ = build(cfg, QUANTS["fp8"], dev)
    # the regional helpers' inputs: 32 text rows + two regions' 16, so that the masked-attention kind shares the shape of the others
    d6 = to_dev(t_reg.region_inputs("plain", cfg.params, 64, 64, 32, 6, seed=5), dev)
    per_sample = lambda n: {k: v[:n] if k not in ("groups", "groups2") else v for k, v in d6.items()}
    d3, d1 = per_sample(3), per_sample(1)
    g = torch.Generator().manual_seed(905)
    dw = dict(d1, canvas=torch.randn(1, HC, WC, 64, generator=g).to(torch.bfloat16).to(dev), win_ids=d1["img_ids"])
    plan = make_plan((3, 3))  # 2 x 3 windows: six samples
    ts = fo.get_schedule(16, d6["img"].shape[1])
    lat = plain_denoise(model, d6, ts[:14], use_graph=False)  # a long plain request freezes the scales
    assert model.calibration_state()[0]
    ts2 = ts[:7]  # six steps
    inp = iu.make_inpaint(6, d6["img"].shape[1], 64, 5, device=dev)
    thr = [0.5] * (len(ts2) - 1)
    ids = t_sto.ids_for(11, 6)
    kinds = [
        ("plain", lambda **kw: plain_denoise(model, d6, ts2, img=lat, **kw)),
        ("guided", lambda **kw: guided_denoise(model, d3, ts2, img=lat[:3], **kw)),
        ("shaped", lambda **kw: shaped_denoise(model, d3, ts2, SHAPINGS["apg"], img=lat[:3], **kw)),
        ("blend", lambda **kw: t_inp.denoise(model, d6, ts2, img=lat, inp=inp, **kw)),
        ("differential", lambda **kw: t_inp.denoise(model, d6, ts2, img=lat, inp=inp, thr=thr, **kw)),
        ("solver", lambda **kw: t_sol.denoise(model, d6, ts2, "dpmpp_2m", img=lat, **kw)),
        ("solver_noise", lambda **kw: t_sto.denoise(model, d6, ts2, "euler_ancestral", ids=ids, img=lat, **kw)),
        ("edit", lambda **kw: run_edit(model, d3, ts2, x0=lat[:3], **kw)),
        ("windowed", lambda **kw: run_windows(model, dw, plan, ts2, **kw)),
        ("previewed", lambda **kw: t_pv.denoise(model, d6, ts2, img=lat, preview=t_pv.call(t_pv.Collector(), every=1, n=6), **kw)),
        ("masked_attention", lambda **kw: t_reg.denoise(model, d6, ts2, img=lat, **kw)),
    ]
    first, counts = {}, []
    for rnd in range(2):
        for name, run in kinds:
            c0 = captures(model)
            got = run()
            c1 = captures(model)
            assert c1 > c0, f"round {rnd}: {name} replayed the graph of the kind before it"
            again = run()
            assert captures(model) == c1, f"round {rnd}: an immediate repeat of {name} re-captured"
            ref = first.setdefault(name, got)
            for what, t in (("visit", got), ("repeat", again)):
                assert torch.equal(t, ref), f"round {rnd}: {name} ({what}) differs from its own first result: rel-L2 {rel_l2(t, ref):.3e}"
            counts.append(c1)
    assert torch.equal(first["previewed"], first["plain"]), "the preview launch changed the latents"
    assert len({v.cpu().view(torch.int16).numpy().tobytes() for v in first.values()}) == len(kinds) - 1, "two kinds gave the same bits"
    for name, run in kinds:
        eager = run(use_graph=False)
        assert torch.equal(eager, first[name]), f"{name}: graph vs eager: rel-L2 {rel_l2(eager, first[name]):.3e}"
    n = C.c_longlong(0)
    _lib.call("fluxmi_engine_workspace_bytes", model._engine, C.byref(n))
    print("captures:", " ".join(str(c) for c in counts))
    print("workspace_bytes:", n.value)
    want_counts, want_bytes = recorded()
    assert counts == want_counts, "the capture counts after each visit differ from the recorded sequence"
    assert n.value == want_bytes, f"the engine owns {n.value} bytes after the sequence, {want_bytes} recorded"
