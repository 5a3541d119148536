"""Masked-latent inpainting and differential diffusion, host side: the mask preparation, the threshold table and its slices, the fp32 rounding
model of the blend against the torch expression, what a request without a mask passes on, the ctypes table, the HTTP fields, and the
inpainting state riding in the one request broadcast (gloo, world 2).  No GPU."""
import io
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import inpaint_util as iu

H, W = 96, 64


class StubFlow:
    """records every denoise call with ALL its keyword arguments; a per-sample function of its inputs"""

    def __init__(self):
        self.calls = []

    def denoise(self, img, img_ids, txt, txt_ids, vec, timesteps, **kw):
        self.calls.append(dict(kw, img=img, ts=list(timesteps), txt=txt))
        out = img.float() * 2 + txt.float().mean(dim=(1, 2), keepdim=True) + len(timesteps)
        if "inpaint_mask" in kw:
            out = out * kw["inpaint_mask"].float() + kw["inpaint_x0"].float()
        return out.to(img.dtype)


class StubAE:
    """a deterministic 'encoder': 8 x 8 block means of the three colour planes, tiled over 16 latent channels"""

    def encode(self, x, noise=None):
        z = torch.nn.functional.avg_pool2d(x.float(), 8)
        return torch.cat([z * (i + 1) for i in range(6)], 1)[:, :16].to(torch.bfloat16)


def make_pipe(model=None):
    from flux_pipeline import FluxPipeline

    pipe = FluxPipeline.__new__(FluxPipeline)
    pipe.name, pipe.debug, pipe.dtype, pipe.ae_dtype = "flux-dev", False, torch.bfloat16, torch.bfloat16
    pipe.device_flux = pipe.device_ae = pipe.device_clip = pipe.device_t5 = torch.device("cpu")
    pipe.model, pipe.ae, pipe.clip, pipe.t5, pipe.rng = model or StubFlow(), StubAE(), None, None, torch.Generator(device="cpu")
    pipe.redux = None
    return pipe


def embeddings(batch, seed, Lt=6):
    g = torch.Generator().manual_seed(seed)
    return {"txt": torch.randn(batch, Lt, 16, generator=g), "vec": torch.randn(batch, 8, generator=g)}


def photo(seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def box_mask():
    m = np.zeros((H, W), dtype=np.uint8)
    m[24:72, 16:48] = 255
    return m


KW = dict(width=W, height=H, num_steps=8, seed=11, output_type="latent", silent=True)


# ---- the mask ---------------------------------------------------------------------------------------------------------------------------
def test_mask_preparation_block_means_binarisation_and_packing():
    from flux_pipeline import FluxPipeline

    pipe = make_pipe()
    m = np.zeros((H, W), dtype=np.uint8)
    m[0:8, 0:8] = 255                       # latent pixel (0, 0): all white
    m[0:4, 8:16] = 255                      # (0, 1): exactly half  -> regenerate (>= 0.5)
    blk = m[8:16, 0:8].copy().reshape(-1)
    blk[:31] = 255                          # (1, 0): 31 of 64     -> keep
    m[8:16, 0:8] = blk.reshape(8, 8)
    m[16:24, 8:16] = 128                    # (2, 1): grey 128 / 255 = 0.50196 -> regenerate
    m[16:24, 0:8] = 127                     # (2, 0): grey 127 / 255 = 0.498   -> keep
    lat = torch.zeros(1, 1, H // 8, W // 8)
    lat[0, 0, 0, 0] = lat[0, 0, 0, 1] = lat[0, 0, 2, 1] = 1.0
    want = FluxPipeline.pack(lat.repeat(1, 16, 1, 1)).to(torch.bfloat16)
    got = pipe.prepare_inpaint_mask(m, H, W)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (1, (H // 16) * (W // 16), 64)
    assert torch.equal(got, want)
    # differential: the block means themselves
    lat_d = torch.zeros(1, 1, H // 8, W // 8)
    lat_d[0, 0, 0, 0], lat_d[0, 0, 0, 1], lat_d[0, 0, 1, 0], lat_d[0, 0, 2, 1], lat_d[0, 0, 2, 0] = 1.0, 0.5, 31 / 64, 128 / 255, 127 / 255
    got_d = pipe.prepare_inpaint_mask(m, H, W, differential=True)
    assert torch.equal(got_d, FluxPipeline.pack(lat_d.repeat(1, 16, 1, 1)).to(torch.bfloat16))
    # an RGB mask goes through "L"; another size is resized and centre-cropped like the init image
    assert torch.equal(pipe.prepare_inpaint_mask(np.repeat(m[..., None], 3, -1), H, W), want)
    big = pipe.prepare_inpaint_mask(np.kron(box_mask(), np.ones((2, 2), dtype=np.uint8)), H, W)
    assert torch.equal(big, pipe.prepare_inpaint_mask(box_mask(), H, W))
    for bad in (1.5, torch.zeros(H, W), None):
        with pytest.raises(TypeError, match="inpaint_mask"):
            pipe.prepare_inpaint_mask(bad, H, W)


# ---- the request ------------------------------------------------------------------------------------------------------------------------
def test_generate_passes_latent_noise_mask_and_threshold_slices():
    from flux_pipeline import FluxPipeline

    pos, neg = embeddings(1, 1), embeddings(1, 2)
    ph, mk = photo(), box_mask()
    pipe = make_pipe()
    pipe.generate(pos, init_image=ph, inpaint_mask=mk, **KW)
    (c,) = pipe.model.calls
    x = torch.from_numpy(ph).permute(2, 0, 1).contiguous().to(torch.bfloat16).div(127.5).sub(1)[None]
    x0 = FluxPipeline.pack(StubAE().encode(x))
    assert torch.equal(c["inpaint_x0"], x0) and "inpaint_thresholds" not in c and len(c["ts"]) == 9
    assert torch.equal(c["inpaint_mask"], pipe.prepare_inpaint_mask(mk, H, W))
    assert torch.equal(c["inpaint_noise"], c["img"]), "at strength 1 the request starts from the pure draw"
    noise = c["inpaint_noise"]
    # strength 0.5: 4 of 8 steps run; the start is the blend, `inpaint_noise` stays the pure draw
    pipe = make_pipe()
    pipe.generate(pos, init_image=ph, inpaint_mask=mk, inpaint_differential=True, strength=0.5, **KW)
    (c,) = pipe.model.calls
    assert len(c["ts"]) == 5 and c["inpaint_thresholds"] == [0.75, 0.5, 0.25, 0.0]
    assert torch.equal(c["inpaint_noise"], noise) and torch.equal(c["inpaint_x0"], x0)
    t = c["ts"][0]
    assert torch.equal(c["img"], t * noise + (1.0 - t) * x0)
    assert torch.equal(c["inpaint_mask"], pipe.prepare_inpaint_mask(mk, H, W, differential=True))
    # the table is sliced over the denoise calls of a true_cfg_interval request; each slice is as long as its call
    pipe = make_pipe()
    pipe.generate(pos, init_image=ph, inpaint_mask=mk, inpaint_differential=True, negative_prompt=neg, true_cfg_scale=3.5,
                  true_cfg_interval=(0.25, 0.75), **KW)
    thr = FluxPipeline.inpaint_thresholds(8)
    assert thr == [1.0 - (i + 1) / 8 for i in range(8)] and thr[-1] == 0.0
    assert [c["inpaint_thresholds"] for c in pipe.model.calls] == [thr[0:2], thr[2:6], thr[6:8]]
    assert [len(c["ts"]) - 1 for c in pipe.model.calls] == [2, 4, 2]
    assert [("neg_txt" in c and c["neg_txt"] is not None) for c in pipe.model.calls] == [False, True, False]
    assert all(torch.equal(c["inpaint_x0"], x0) and torch.equal(c["inpaint_noise"], noise) for c in pipe.model.calls)
    # num_images: one encode, one mask, a noise draw per image
    pipe = make_pipe()
    pipe.generate(embeddings(2, 1), init_image=ph, inpaint_mask=mk, num_images=2, **KW)
    (c,) = pipe.model.calls
    assert c["inpaint_x0"].shape[0] == 2 and torch.equal(c["inpaint_x0"][0], c["inpaint_x0"][1]) and torch.equal(c["inpaint_x0"][:1], x0)
    assert not torch.equal(c["inpaint_noise"][0], c["inpaint_noise"][1]) and torch.equal(c["inpaint_mask"][0], c["inpaint_mask"][1])


def test_generate_without_a_mask_passes_todays_arguments_and_refusals():
    pos = embeddings(1, 1)
    pipe = make_pipe()
    pipe.generate(pos, **KW)
    pipe.generate(pos, init_image=photo(), strength=0.5, **KW)
    for c in pipe.model.calls:
        assert set(c) == {"guidance", "use_graph", "img", "ts", "txt"}, f"a request without inpaint_mask passed {sorted(c)}"
    # preprocess_latent returns what it returned: (x, timesteps), the blend at the start time
    g = torch.Generator().manual_seed(3)
    x, ts, lat, noise = pipe.preprocess_latent_parts(torch.from_numpy(photo()), H, W, 8, 0.5, g)
    g = torch.Generator().manual_seed(3)
    x2, ts2 = pipe.preprocess_latent(torch.from_numpy(photo()), H, W, 8, 0.5, g)
    assert torch.equal(x, x2) and ts == ts2 and len(ts) == 5 and torch.equal(x, ts[0] * noise + (1.0 - ts[0]) * lat)
    n = len(pipe.model.calls)
    with pytest.raises(ValueError, match="inpaint_mask needs init_image"):
        pipe.generate(pos, inpaint_mask=box_mask(), **KW)
    with pytest.raises(ValueError, match="inpaint_differential needs an inpaint_mask"):
        pipe.generate(pos, init_image=photo(), inpaint_differential=True, **KW)
    with pytest.raises(TypeError, match="inpaint_mask"):
        pipe.generate(pos, init_image=photo(), inpaint_mask=0.5, **KW)
    with pytest.raises(ValueError, match="need a FLUX.1 Fill"):
        pipe.generate(pos, init_image=photo(), mask_image=box_mask(), **KW)
    assert len(pipe.model.calls) == n, "a refused request reached the flow model"


def test_denoise_validates_the_inpainting_tensors_before_any_device_work():
    import util
    from fluxmi import synth

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    p = cfg.params
    p.hidden_size, p.num_heads, p.depth, p.depth_single_blocks, p.context_in_dim, p.vec_in_dim = 256, 2, 1, 1, 128, 64
    model = util.load_flow_model(cfg, synth.make_state_dict(p, seed=0))
    B, Li, Lt = 2, 4, 6
    img, ids = torch.zeros(B, Li, 64), torch.zeros(B, Li, 3)
    txt, tids, y = torch.zeros(B, Lt, 128), torch.zeros(B, Lt, 3), torch.zeros(B, 64)
    ts = [1.0, 0.5, 0.0]
    t = torch.zeros(B, Li, 64)
    call = lambda **kw: model.denoise(img, ids, txt, tids, y, ts, **kw)
    for kw in (dict(inpaint_x0=t), dict(inpaint_x0=t, inpaint_noise=t), dict(inpaint_mask=t), dict(inpaint_noise=t, inpaint_mask=t)):
        with pytest.raises(ValueError, match="go together"):
            call(**kw)
    with pytest.raises(ValueError, match="inpaint_x0"):
        call(inpaint_x0=t[:1], inpaint_noise=t, inpaint_mask=t)
    with pytest.raises(ValueError, match="inpaint_noise"):
        call(inpaint_x0=t, inpaint_noise=t[..., :32], inpaint_mask=t)
    with pytest.raises(ValueError, match="inpaint_mask"):
        call(inpaint_x0=t, inpaint_noise=t, inpaint_mask=torch.zeros(3, Li, 64))
    with pytest.raises(ValueError, match="inpaint_mask"):
        call(inpaint_x0=t, inpaint_noise=t, inpaint_mask=torch.zeros(Li, 64))
    with pytest.raises(ValueError, match="inpaint_thresholds"):
        call(inpaint_x0=t, inpaint_noise=t, inpaint_mask=t[:1], inpaint_thresholds=[0.5])
    with pytest.raises(ValueError, match="inpaint_thresholds"):
        call(inpaint_x0=t, inpaint_noise=t, inpaint_mask=t[:1], inpaint_thresholds=[0.5, float("nan")])
    with pytest.raises(ValueError, match="inpaint_thresholds"):
        call(inpaint_thresholds=[0.5, 0.0])
    assert model._engine is None, "a refused request created the engine"


def test_chunked_batches_carry_the_inpainting_state():
    """a batch above the engine's cap runs as equal passes (Flux.denoise, `pick`): x0, noise and the mask -- given for batch 1, so it arrives
    expanded -- are sliced and padded like img, the thresholds pass through unchanged.  The single pass is stubbed; no device."""
    import util
    from fluxmi import synth

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    p = cfg.params
    p.hidden_size, p.num_heads, p.depth, p.depth_single_blocks, p.context_in_dim, p.vec_in_dim = 256, 2, 1, 1, 128, 64
    model = util.load_flow_model(cfg, synth.make_state_dict(p, seed=0))
    model.MAX_ENGINE_BATCH = 2
    whole, calls = model.denoise, []

    def single_pass(img, img_ids, txt, txt_ids, y, timesteps, **kw):
        if img.shape[0] > 2:
            return whole(img, img_ids, txt, txt_ids, y, timesteps, **kw)
        calls.append(dict(kw, img=img.clone(), txt=txt.clone()))
        return img + 1

    model.denoise = single_pass  # the passes of the chunked path call self.denoise
    B, Li, Lt = 5, 4, 6
    tag = lambda t: t + torch.arange(B, dtype=torch.float32).reshape(B, *([1] * (t.ndim - 1)))  # sample b carries b
    img, ids = tag(torch.zeros(B, Li, 64)), torch.zeros(B, Li, 3)
    txt, tids, y = tag(torch.zeros(B, Lt, 128)), torch.zeros(B, Lt, 3), torch.zeros(B, 64)
    x0, noise = tag(torch.full((B, Li, 64), 100.0)), tag(torch.full((B, Li, 64), 200.0))
    mask = torch.rand(1, Li, 64, generator=torch.Generator().manual_seed(1))
    ts, thr = [1.0, 0.5, 0.0], [0.5, 0.0]
    out = model.denoise(img, ids, txt, tids, y, ts, inpaint_x0=x0, inpaint_noise=noise, inpaint_mask=mask, inpaint_thresholds=thr)
    assert torch.equal(out, img + 1)
    assert len(calls) == 3
    for c, rows in zip(calls, ([0, 1], [2, 3], [4, 4])):  # 5 = 2 + 2 + (1 padded with a copy of its last sample)
        assert torch.equal(c["img"], img[rows]) and torch.equal(c["txt"], txt[rows])
        assert torch.equal(c["inpaint_x0"], x0[rows]) and torch.equal(c["inpaint_noise"], noise[rows])
        assert tuple(c["inpaint_mask"].shape) == (2, Li, 64) and torch.equal(c["inpaint_mask"], mask.expand(2, -1, -1))
        assert c["inpaint_thresholds"] == thr
    # a per-sample mask is sliced like the rest; without a state the passes get none of the four arguments
    calls.clear()
    masks = tag(torch.zeros(B, Li, 64))
    model.denoise(img, ids, txt, tids, y, ts, inpaint_x0=x0, inpaint_noise=noise, inpaint_mask=masks)
    assert [c["inpaint_mask"][:, 0, 0].tolist() for c in calls] == [[0.0, 1.0], [2.0, 3.0], [4.0, 4.0]]
    assert all(c["inpaint_thresholds"] is None for c in calls)
    calls.clear()
    model.denoise(img, ids, txt, tids, y, ts)
    assert len(calls) == 3 and not any(k.startswith("inpaint") for c in calls for k in c)


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------
def test_fp32_rounding_model_equals_the_torch_expression():
    g = torch.Generator().manual_seed(4)
    shape = (3, 15, 64)
    x, v, x0, noise = (torch.randn(*shape, generator=g).to(torch.bfloat16) for _ in range(4))
    soft = torch.rand(*shape, generator=g).to(torch.bfloat16)
    soft[..., 0], soft[..., 1], soft[..., 2] = 0.5, 0.30078125, 0.298828125
    masks = {"soft": soft, "ones": torch.ones_like(soft), "zeros": torch.zeros_like(soft), "binary": (soft > 0.5).to(torch.bfloat16)}
    for dt, tn in ((-0.0625, 0.7313), (-0.03173828125, 0.40625), (-0.0471, 0.1 + 0.2), (-0.11, 0.0)):
        x1 = x + dt * v
        p = tn * noise + (1.0 - tn) * x0
        for name, m in masks.items():
            for thr in (None, 0.3, 0.5, 0.0, 1.0):
                want = iu.blend_step(x, v, dt, tn, x0, noise, m, thr=thr)
                assert want.dtype == torch.bfloat16
                got = iu.blend_step_fp32_model(x, v, dt, tn, x0, noise, m, thr=thr)
                assert torch.equal(got, want), f"mask {name} dt {dt} t_next {tn} thr {thr}"
                me = iu.effective_mask(m, thr)
                assert torch.equal(want[me == 1], x1[me == 1]), "m == 1 must give x1"
                assert torch.equal(want[me == 0], p[me == 0]), "m == 0 must give p"
                if tn == 0.0:
                    assert torch.equal(want[me == 0], x0[me == 0]), "m == 0 at t_next == 0 must give x0"
    # the compare is the fp32 one: bf16(0.3) = 0.30078125 lies above the fp32 threshold 0.3, 0.298828125 below; equality is no release
    m = torch.tensor([0.30078125, 0.298828125, 0.5, 0.0, 1.0], dtype=torch.bfloat16)
    assert iu.effective_mask(m, 0.3).tolist() == [1.0, 0.0, 1.0, 0.0, 1.0]
    assert iu.effective_mask(m, 0.5).tolist() == [0.0, 0.0, 0.0, 0.0, 1.0]
    assert iu.effective_mask(m, 0.0).tolist() == [1.0, 1.0, 1.0, 0.0, 1.0]


# ---- the interfaces ---------------------------------------------------------------------------------------------------------------------
def test_ctypes_table_has_the_inpainting_entries():
    from fluxmi import _lib

    assert "fluxmi_blend_euler" in _lib.EXPORTS and "fluxmi_engine_set_inpaint" in _lib.EXPORTS
    assert len(_lib.lib.fluxmi_blend_euler.argtypes) == len(_lib.lib.fluxmi_cfg_euler.argtypes) + 6  # x0, noise, mask, tnext, 1 - tnext, thr
    assert len(_lib.lib.fluxmi_engine_set_inpaint.argtypes) == 8
    assert _lib.lib.fluxmi_abi_version() == 5 and _lib.ABI_VERSION == 5
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "fluxmi.h")).read()
    assert "int fluxmi_blend_euler(" in header and "int fluxmi_engine_set_inpaint(" in header


def test_http_inpaint_fields():
    """`inpaint_mask` / `inpaint_differential` reach generate() only when set; a request without them produces exactly today's keyword arguments"""
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
    assert c.post("/generate", json={**base, "inpaint_mask": None, "inpaint_differential": None}).status_code == 200
    assert not {"inpaint_mask", "inpaint_differential"} & set(calls[-1])
    r = c.post("/generate", json={**base, "init_image": "photo.png", "inpaint_mask": "mask.png"})
    assert r.status_code == 200 and r.content.startswith(b"\xff\xd8")
    assert calls[-1]["inpaint_mask"] == "mask.png" and calls[-1]["init_image"] == "photo.png" and "inpaint_differential" not in calls[-1]
    assert "mask_image" not in calls[-1]
    r = c.post("/generate", json={**base, "init_image": "photo.png", "inpaint_mask": "mask.png", "inpaint_differential": True})
    assert r.status_code == 200 and calls[-1]["inpaint_differential"] is True
    assert c.post("/generate", json={**base, "inpaint_mask": 3}).status_code == 422
    assert c.post("/generate", json={**base, "inpaint_differential": "maybe"}).status_code == 422


# ---- process groups ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _inpaint_worker(rank, world, port, batch, q):
    import sys

    import torch.distributed as td

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "flux-fp8-api_amd"), os.path.join(root, "tests")):
        sys.path.insert(0, p)
    from fluxmi import dist as fdist
    from test_inpaint_cpu import KW, box_mask, embeddings, make_pipe, photo

    pos = embeddings(batch, 1)
    kw = dict(KW, num_images=batch, inpaint_differential=True)
    single = make_pipe()
    expect = single.generate(pos, init_image=photo(0), inpaint_mask=box_mask(), **kw)  # single process: the whole batch on one replica
    (whole,) = single.model.calls
    plain_single = make_pipe()
    plain_single.generate(pos, **dict(KW, num_images=batch))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    fdist.init_from_env("gloo")
    # what goes over the wire: every flat buffer handed to the collective
    sent, real = [], td.broadcast

    def spy(t, src=0, **kwargs):
        if rank == src:
            sent.append(t.clone())
        return real(t, src=src, **kwargs)

    td.broadcast = spy
    # rank 1 holds ANOTHER photo and ANOTHER mask: what it steps must be rank 0's
    mine = (photo(0), box_mask()) if rank == 0 else (photo(1), np.full_like(box_mask(), 255))
    pipe = make_pipe()
    out = pipe.generate(pos if rank == 0 else {k: torch.zeros_like(v) for k, v in pos.items()}, init_image=mine[0], inpaint_mask=mine[1], **kw)
    lo, hi = fdist.shard_bounds(batch, rank, world)
    calls = pipe.model.calls
    ok = len(calls) == (1 if hi > lo else 0)
    if calls:
        c = calls[0]
        ok = ok and all(torch.equal(c[k], whole[k][lo:hi]) for k in ("inpaint_x0", "inpaint_noise", "inpaint_mask", "img"))
        ok = ok and c["inpaint_thresholds"] == whole["inpaint_thresholds"]
    ok = ok and ((out is not None and torch.equal(out, expect)) if rank == 0 else out is None)
    if rank == 0:
        flat = sent[0]  # the request broadcast comes first (an uneven gather broadcasts shards later)
        n_inp = 3 * whole["inpaint_x0"].numel()
        per_tok = torch.cat((whole["inpaint_x0"], whole["inpaint_noise"], whole["inpaint_mask"]), -1).reshape(-1)
        ok = ok and torch.equal(flat[-n_inp:], per_tok)
        head = flat[:-n_inp].clone()
    # the same request without a mask: the buffer is today's [txt | vec | noise], byte for byte
    sent.clear()
    pipe = make_pipe()
    pipe.generate(pos if rank == 0 else {k: torch.zeros_like(v) for k, v in pos.items()}, **dict(KW, num_images=batch))
    if rank == 0:
        flat = sent[0]
        (pc,) = plain_single.model.calls
        today = torch.cat([pos["txt"].bfloat16().reshape(-1), pos["vec"].bfloat16().reshape(-1), pc["img"].reshape(-1)])
        ok = ok and flat.dtype == today.dtype and flat.numel() == today.numel() and torch.equal(flat.view(torch.int16), today.view(torch.int16))
        ok = ok and torch.equal(head[:pos["txt"].numel() + pos["vec"].numel()], today[:pos["txt"].numel() + pos["vec"].numel()])
    td.broadcast = real
    q.put((rank, bool(ok), (lo, hi)))
    td.barrier()
    td.destroy_process_group()


@pytest.mark.parametrize("batch", [1, 3])
def test_broadcast_request_carries_the_inpainting_state_over_gloo(batch):
    """FluxPipeline.generate with an inpaint_mask under a 2-rank process group: rank 0's [x0 | noise | mask] rides behind [txt | vec | noise]
    in the ONE broadcast and is sharded like the images, so each rank blends with rank 0's latent and mask for exactly its images; without
    a mask the buffer is today's, byte for byte.  batch 1 < world 2: the rank with the empty shard joins the collectives and denoises nothing."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_inpaint_worker, args=(r, 2, port, batch, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok, _ in res), res


def test_broadcast_request_without_a_process_group_returns_its_parts():
    from fluxmi import dist as fdist

    a, b, c, d, e = (torch.full((2, 3), float(i)) for i in range(5))
    assert len(fdist.broadcast_request(a, b, c)) == 3
    assert fdist.broadcast_request(a, b, c, extra=d)[3] is d
    assert fdist.broadcast_request(a, b, c, inpaint=e)[3] is e
    out = fdist.broadcast_request(a, b, c, extra=d, inpaint=e)
    assert len(out) == 5 and out[3] is d and out[4] is e
