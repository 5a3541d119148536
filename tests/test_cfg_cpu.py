"""Negative prompts (true classifier-free guidance), host side: argument validation of FluxPipeline.generate / Flux.denoise that needs no
device, which calls a request turns into (guided or not, interval segments, draw order), the HTTP fields, and the negative embeddings
riding in the one request broadcast (gloo, world 2) with both branches of an image on the rank that owns the image.  No GPU."""
import io
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp


class StubFlow:
    """records every denoise call; a per-sample function of its inputs, the negative branch included"""

    def __init__(self):
        self.calls = []

    def denoise(self, img, img_ids, txt, txt_ids, vec, timesteps, guidance=3.5, use_graph=True, neg_txt=None, neg_y=None, cfg_scale=1.0):
        self.calls.append(dict(B=img.shape[0], ts=list(timesteps), neg_txt=neg_txt, neg_y=neg_y, cfg_scale=cfg_scale, txt=txt, vec=vec, img=img))
        assert img_ids.shape[0] == txt.shape[0] == txt_ids.shape[0] == vec.shape[0] == img.shape[0]
        out = img.float() * 2 + txt.float().mean(dim=(1, 2), keepdim=True) + vec.float().sum(-1)[:, None, None] + len(timesteps)
        if neg_txt is not None:
            assert neg_txt.shape == txt.shape and neg_y.shape == vec.shape
            out = out + cfg_scale * (neg_txt.float().mean(dim=(1, 2), keepdim=True) - neg_y.float().sum(-1)[:, None, None])
        return out.to(img.dtype)


def make_pipe(model=None):
    from flux_pipeline import FluxPipeline

    pipe = FluxPipeline.__new__(FluxPipeline)
    pipe.name, pipe.debug, pipe.dtype, pipe.ae_dtype = "flux-dev", False, torch.bfloat16, torch.bfloat16
    pipe.device_flux = pipe.device_ae = pipe.device_clip = pipe.device_t5 = torch.device("cpu")
    pipe.model, pipe.ae, pipe.clip, pipe.t5, pipe.rng = model or StubFlow(), None, None, None, torch.Generator(device="cpu")
    pipe.redux = None
    return pipe


def embeddings(batch, seed, Lt=6):
    g = torch.Generator().manual_seed(seed)
    return {"txt": torch.randn(batch, Lt, 16, generator=g), "vec": torch.randn(batch, 8, generator=g)}


KW = dict(width=64, height=96, num_steps=8, seed=11, output_type="latent", silent=True)


def test_generate_guides_iff_a_negative_prompt_and_a_scale_above_one():
    pos, neg = embeddings(1, 1), embeddings(1, 2)
    pipe = make_pipe()
    plain = pipe.generate(pos, **KW)
    assert len(pipe.model.calls) == 1 and pipe.model.calls[0]["neg_txt"] is None
    noise = pipe.model.calls[0]["img"]
    # a negative prompt with scale <= 1: today's call; the negative prompt is not even looked at
    for extra in (dict(negative_prompt=neg), dict(negative_prompt=neg, true_cfg_scale=1.0), dict(negative_prompt={"junk": 0}, true_cfg_scale=0.5)):
        pipe = make_pipe()
        assert torch.equal(pipe.generate(pos, **extra, **KW), plain)
        assert len(pipe.model.calls) == 1 and pipe.model.calls[0]["neg_txt"] is None
    pipe = make_pipe()
    out = pipe.generate(pos, negative_prompt=neg, true_cfg_scale=3.5, **KW)
    (c,) = pipe.model.calls
    assert c["cfg_scale"] == 3.5 and len(c["ts"]) == 9
    assert torch.equal(c["neg_txt"], neg["txt"].bfloat16()) and torch.equal(c["neg_y"], neg["vec"].bfloat16())
    assert torch.equal(c["img"], noise), "a seed must draw the same noise with and without a negative prompt"
    assert out.shape == plain.shape and not torch.equal(out, plain)


def test_generate_refuses_a_scale_without_a_negative_prompt_and_malformed_requests():
    pos, neg = embeddings(2, 1), embeddings(2, 2)
    pipe = make_pipe()
    with pytest.raises(ValueError, match="needs a negative_prompt"):
        pipe.generate(pos, true_cfg_scale=2.0, num_images=2, **KW)
    with pytest.raises(ValueError, match="sequence length"):
        pipe.generate(pos, negative_prompt=embeddings(2, 2, Lt=5), true_cfg_scale=2.0, num_images=2, **KW)
    with pytest.raises(ValueError, match="negative prompts for a batch"):
        pipe.generate(pos, negative_prompt=["a", "b", "c"], true_cfg_scale=2.0, num_images=2, **KW)
    for bad in ((0.5, 0.25), (-0.1, 1.0), (0.0, 1.5), 0.5, (0.1, 0.2, 0.3)):
        with pytest.raises(ValueError, match="true_cfg_interval"):
            pipe.generate(pos, negative_prompt=neg, true_cfg_scale=2.0, true_cfg_interval=bad, num_images=2, **KW)
    assert pipe.model.calls == [], "a refused request reached the flow model"
    # one negative embedding is shared by the batch
    pipe.generate(pos, negative_prompt=embeddings(1, 3), true_cfg_scale=2.0, num_images=2, **KW)
    c = pipe.model.calls[-1]
    assert c["neg_txt"].shape == c["txt"].shape and torch.equal(c["neg_txt"][0], c["neg_txt"][1])


@pytest.mark.parametrize("interval, want", [
    ((0.0, 1.0), [(0, 8, True)]),
    ((0.25, 0.75), [(0, 2, False), (2, 6, True), (6, 8, False)]),
    ((0.0, 0.5), [(0, 4, True), (4, 8, False)]),
    ((0.3, 1.0), [(0, 3, False), (3, 8, True)]),       # 0.3 * 8 = 2.4 <= i  ->  i >= 3
    ((0.0, 0.3), [(0, 3, True), (3, 8, False)]),       # i < 2.4  ->  i <= 2
    ((0.0, 0.0), [(0, 8, False)]),
    ((0.5, 0.5), [(0, 8, False)]),
    ((0.3, 0.35), [(0, 8, False)]),                    # no integer step in [2.4, 2.8)
])
def test_true_cfg_interval_becomes_consecutive_denoise_calls(interval, want):
    pos, neg = embeddings(1, 1), embeddings(1, 2)
    ref = make_pipe()
    ref.generate(pos, **KW)
    ts = ref.model.calls[0]["ts"]
    assert len(ts) == 9
    pipe = make_pipe()
    pipe.generate(pos, negative_prompt=neg, true_cfg_scale=3.5, true_cfg_interval=interval, **KW)
    got = [(ts.index(c["ts"][0]), ts.index(c["ts"][-1]), c["neg_txt"] is not None) for c in pipe.model.calls]
    assert got == want
    assert all(c["ts"] == ts[a:b + 1] for c, (a, b, _) in zip(pipe.model.calls, want))
    for prev, nxt in zip(pipe.model.calls[:-1], pipe.model.calls[1:]):  # each segment starts from the previous one's latents
        assert nxt["img"].shape == prev["img"].shape and not torch.equal(nxt["img"], prev["img"])


def test_redux_tokens_go_to_both_branches():
    """the image tokens are appended behind the T5 tokens of the prompt AND of the negative prompt (the encoder runs once)"""
    import numpy as np

    class StubRedux:
        num_tokens, calls = 5, 0

        def __call__(self, images):
            StubRedux.calls += 1
            return (torch.arange(len(images) * 5 * 16, dtype=torch.float32).view(len(images), 5, 16) / 7).to(torch.bfloat16)

    pos, neg = embeddings(2, 1), embeddings(1, 2)
    pipe = make_pipe()
    pipe.redux = StubRedux()
    pipe.generate(pos, negative_prompt=neg, true_cfg_scale=2.0, num_images=2, redux_image=np.zeros((8, 8, 3), dtype=np.uint8), **KW)
    (c,) = pipe.model.calls
    assert StubRedux.calls == 1 and c["txt"].shape == (2, 6 + 5, 16) and c["neg_txt"].shape == c["txt"].shape
    assert torch.equal(c["txt"][:, :6], pos["txt"].bfloat16()) and torch.equal(c["neg_txt"][:, :6], neg["txt"].bfloat16().expand(2, -1, -1))
    assert torch.equal(c["neg_txt"][:, 6:], c["txt"][:, 6:]) and c["txt"][:, 6:].abs().sum() > 0


def test_denoise_validates_the_negative_pair_before_any_device_work():
    import util

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    p = cfg.params
    p.hidden_size, p.num_heads, p.depth, p.depth_single_blocks, p.context_in_dim, p.vec_in_dim = 256, 2, 1, 1, 128, 64
    from fluxmi import synth

    model = util.load_flow_model(cfg, synth.make_state_dict(p, seed=0))
    B, Li, Lt = 2, 4, 6
    img, ids = torch.zeros(B, Li, 64), torch.zeros(B, Li, 3)
    txt, tids, y = torch.zeros(B, Lt, 128), torch.zeros(B, Lt, 3), torch.zeros(B, 64)
    ts = [1.0, 0.5, 0.0]
    call = lambda **kw: model.denoise(img, ids, txt, tids, y, ts, **kw)
    with pytest.raises(ValueError, match="go together"):
        call(neg_txt=txt)
    with pytest.raises(ValueError, match="go together"):
        call(neg_y=y)
    with pytest.raises(ValueError, match="sequence length"):
        call(neg_txt=torch.zeros(B, Lt + 1, 128), neg_y=y)
    with pytest.raises(ValueError, match="neg_txt"):
        call(neg_txt=torch.zeros(B, Lt, 64), neg_y=y)
    with pytest.raises(ValueError, match="neg_txt"):
        call(neg_txt=torch.zeros(3, Lt, 128), neg_y=y)
    with pytest.raises(ValueError, match="neg_y"):
        call(neg_txt=txt, neg_y=torch.zeros(B, 32))
    with pytest.raises(ValueError, match="neg_y"):
        call(neg_txt=txt[:1], neg_y=torch.zeros(3, 64))
    assert model._engine is None, "a refused request created the engine"


def test_ctypes_table_has_the_guided_entries():
    from fluxmi import _lib

    assert "fluxmi_cfg_euler" in _lib.EXPORTS and "fluxmi_engine_denoise_cfg" in _lib.EXPORTS
    assert len(_lib.lib.fluxmi_engine_denoise_cfg.argtypes) == len(_lib.lib.fluxmi_engine_denoise.argtypes) + 1
    assert _lib.lib.fluxmi_abi_version() == 5


def test_http_negative_prompt_fields():
    """`negative_prompt` / `true_cfg_scale` / `true_cfg_interval` reach generate() only when set; a request without them produces exactly
    today's keyword arguments."""
    from fastapi.testclient import TestClient

    import api

    calls = []

    class Stub:
        def generate(self, **kw):
            calls.append(kw)
            return io.BytesIO(b"\xff\xd8jpeg-bytes\xff\xd9")

    api.app.state.model = Stub()
    c = TestClient(api.app)
    base = {"prompt": "a cat on a bench", "width": 512, "height": 512, "num_steps": 4, "seed": 7}
    assert c.post("/generate", json=base).status_code == 200
    assert set(calls[-1]) == {"prompt", "width", "height", "num_steps", "guidance", "seed", "strength", "init_image"}
    assert c.post("/generate", json={**base, "negative_prompt": None, "true_cfg_scale": None, "true_cfg_interval": None}).status_code == 200
    assert not {"negative_prompt", "true_cfg_scale", "true_cfg_interval"} & set(calls[-1])
    r = c.post("/generate", json={**base, "negative_prompt": "", "true_cfg_scale": 3.5})
    assert r.status_code == 200 and r.content.startswith(b"\xff\xd8")
    assert calls[-1]["negative_prompt"] == "" and calls[-1]["true_cfg_scale"] == 3.5 and "true_cfg_interval" not in calls[-1]
    r = c.post("/generate", json={**base, "negative_prompt": "blurry, (low quality:1.3)", "true_cfg_scale": 4, "true_cfg_interval": [0.0, 0.5]})
    assert r.status_code == 200 and calls[-1]["negative_prompt"] == "blurry, (low quality:1.3)" and calls[-1]["true_cfg_scale"] == 4.0
    assert tuple(calls[-1]["true_cfg_interval"]) == (0.0, 0.5)
    assert c.post("/generate", json={**base, "true_cfg_interval": [0.1]}).status_code == 422
    assert c.post("/generate", json={**base, "negative_prompt": 3}).status_code == 422


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _guided_worker(rank, world, port, batch, q):
    import sys

    import torch.distributed as td

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "flux-fp8-api_amd"), os.path.join(root, "tests")):
        sys.path.insert(0, p)
    from fluxmi import dist as fdist
    from test_cfg_cpu import KW, embeddings, make_pipe

    # image b's prompt is marked b + 1, its negative prompt -(b + 1): a branch on the wrong rank (or beside the wrong image) shows
    pos, neg = embeddings(batch, 1), embeddings(batch, 2)
    for b in range(batch):
        pos["txt"][b, 0, 0], neg["txt"][b, 0, 0] = b + 1, -(b + 1)
    kw = dict(KW, num_images=batch)
    gkw = dict(true_cfg_scale=3.5, true_cfg_interval=(0.0, 0.5))
    expect = make_pipe().generate(pos, negative_prompt=neg, **gkw, **kw)  # single process: the whole batch on one replica
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    fdist.init_from_env("gloo")
    mine_pos, mine_neg = (pos, neg) if rank == 0 else ({k: torch.zeros_like(v) for k, v in pos.items()}, {k: torch.zeros_like(v) for k, v in neg.items()})
    pipe = make_pipe()
    out = pipe.generate(mine_pos, negative_prompt=mine_neg, **gkw, **kw)
    lo, hi = fdist.shard_bounds(batch, rank, world)
    calls = pipe.model.calls
    ok = [c["B"] for c in calls] == ([hi - lo, hi - lo] if hi > lo else [])  # guided half, plain half; an empty shard skips both
    if calls:
        g = calls[0]
        ok = ok and g["neg_txt"] is not None and calls[1]["neg_txt"] is None
        ok = ok and torch.equal(g["txt"], pos["txt"][lo:hi].bfloat16()) and torch.equal(g["vec"], pos["vec"][lo:hi].bfloat16())
        ok = ok and torch.equal(g["neg_txt"], neg["txt"][lo:hi].bfloat16()) and torch.equal(g["neg_y"], neg["vec"][lo:hi].bfloat16())
        ok = ok and [float(v) for v in g["txt"][:, 0, 0]] == [float(b + 1) for b in range(lo, hi)]
        ok = ok and [float(v) for v in g["neg_txt"][:, 0, 0]] == [-float(b + 1) for b in range(lo, hi)]
    ok = ok and ((out is not None and torch.equal(out, expect)) if rank == 0 else out is None)
    q.put((rank, bool(ok), (lo, hi)))
    td.barrier()
    td.destroy_process_group()


@pytest.mark.parametrize("batch", [1, 3])
def test_broadcast_request_carries_the_negative_embeddings_over_gloo(batch):
    """FluxPipeline.generate with a negative prompt under a 2-rank process group: rank 0's [txt; neg_txt] and [vec; neg_vec] ride in the one
    broadcast, images (not branches) are sharded, so each rank's denoise gets the prompt AND the negative prompt of exactly its images, and
    rank 0 gathers what a single replica produces.  batch 1 < world 2: the rank with the empty shard joins the collectives and skips both
    segments."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_guided_worker, args=(r, 2, port, batch, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok, _ in res), res
