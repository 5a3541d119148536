"""FLUX.1 Kontext reference-image editing, host side: the resolution snap and latent sizes of the reference, its position ids, the HTTP
field and the reference latents riding in the one request broadcast (gloo, world 2).  No GPU."""
import io
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp


@pytest.mark.parametrize("size, snapped, latent, Lc", [
    ((1920, 1080), (1392, 752), (174, 94), 4089),   # odd Lc
    ((800, 1200), (832, 1248), (104, 156), 4056),
    ((1024, 1024), (1024, 1024), (128, 128), 4096),
    ((37, 37), (1024, 1024), (128, 128), 4096),
    ((4000, 4000), (1024, 1024), (128, 128), 4096),
    ((100, 10000), (672, 1568), (84, 196), 4116),    # extreme portrait: the narrowest preferred size
    ((10000, 100), (1568, 672), (196, 84), 4116),    # extreme landscape
    ((1, 2), (720, 1456), (90, 182), 4095),          # a = 0.5: the nearest ratio, not the narrowest
])
def test_reference_resolution_snap(size, snapped, latent, Lc):
    from flux_pipeline import kontext_reference_size

    w, h, w_l, h_l = kontext_reference_size(*size)
    assert (w, h) == snapped and (w_l, h_l) == latent
    assert (h_l // 2) * (w_l // 2) == Lc


def test_snap_is_the_stated_min_over_the_list():
    from flux_pipeline import KONTEXT_PREFERRED_RESOLUTIONS, kontext_reference_size

    assert len(KONTEXT_PREFERRED_RESOLUTIONS) == 17 and (1024, 1024) in KONTEXT_PREFERRED_RESOLUTIONS
    for W in range(64, 3000, 97):
        for H in range(64, 3000, 131):
            a = W / H
            best = min((abs(a - w / h), w, h) for (w, h) in KONTEXT_PREFERRED_RESOLUTIONS)
            assert kontext_reference_size(W, H)[:2] == best[1:]


def test_reference_position_ids():
    from flux_pipeline import FluxPipeline, kontext_reference_ids

    h_l, w_l = 6, 10
    ids = kontext_reference_ids(2, h_l, w_l, "cpu", torch.bfloat16)
    assert ids.shape == (2, (h_l // 2) * (w_l // 2), 3) and ids.dtype == torch.bfloat16
    assert (ids[..., 0] == 1).all()
    grid = ids[0].view(h_l // 2, w_l // 2, 3)
    assert torch.equal(grid[..., 1], torch.arange(h_l // 2, dtype=torch.bfloat16)[:, None].expand(h_l // 2, w_l // 2))
    assert torch.equal(grid[..., 2], torch.arange(w_l // 2, dtype=torch.bfloat16)[None, :].expand(h_l // 2, w_l // 2))
    assert torch.equal(ids[0], ids[1])
    plain = FluxPipeline.make_img_ids(2, h_l // 2, w_l // 2, "cpu", torch.bfloat16)
    assert torch.equal(ids[..., 1:], plain[..., 1:]) and (plain[..., 0] == 0).all()
    # the largest grid (a 1568 edge: 98 rows / columns) keeps exact integer ids in bf16
    big = kontext_reference_ids(1, 196, 84, "cpu", torch.bfloat16)
    assert big[0, -1].tolist() == [1.0, 97.0, 41.0]


def test_http_reference_image_field():
    """`reference_image` reaches generate() when set; a request without it produces exactly today's keyword arguments."""
    from fastapi.testclient import TestClient

    import api

    calls = []

    class Stub:
        def generate(self, **kw):
            calls.append(kw)
            return io.BytesIO(b"\xff\xd8jpeg-bytes\xff\xd9")

    api.app.state.model = Stub()
    c = TestClient(api.app)
    base = {"prompt": "make the car red", "width": 512, "height": 512, "num_steps": 4, "seed": 7}
    assert c.post("/generate", json=base).status_code == 200
    assert set(calls[-1]) == {"prompt", "width", "height", "num_steps", "guidance", "seed", "strength", "init_image"}
    assert c.post("/generate", json={**base, "reference_image": None}).status_code == 200
    assert "reference_image" not in calls[-1]
    r = c.post("/generate", json={**base, "reference_image": "car.png"})
    assert r.status_code == 200 and r.content.startswith(b"\xff\xd8")
    assert calls[-1]["reference_image"] == "car.png" and calls[-1]["seed"] == 7 and calls[-1]["init_image"] is None
    r = c.post("/generate", json={**base, "reference_image": "aGVsbG8=", "init_image": "in.png", "strength": 0.5})
    assert r.status_code == 200 and calls[-1]["reference_image"] == "aGVsbG8=" and calls[-1]["init_image"] == "in.png"


def test_broadcast_request_without_a_process_group_passes_extra_through():
    from fluxmi import dist as fdist

    a, b, c, d = torch.zeros(1, 2, 3), torch.ones(1, 4), torch.full((1, 5, 6), 2.0), torch.full((1, 7, 6), 3.0)
    assert fdist.broadcast_request(a, b, c) == (a, b, c)
    assert fdist.broadcast_request(a, b, c, extra=d) == (a, b, c, d)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _broadcast_worker(rank, world, port, q):
    import sys

    import torch.distributed as td

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "flux-fp8-api_amd"))
    from fluxmi import dist as fdist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    fdist.init_from_env("gloo")
    g = torch.Generator().manual_seed(0)
    B = 3
    txt = torch.randn(B, 6, 16, generator=g).bfloat16()
    vec = torch.randn(B, 8, generator=g).bfloat16()
    noise = torch.randn(B, 12, 64, generator=g).bfloat16()
    cond = torch.randn(B, 15, 64, generator=g).bfloat16()  # Lc != Li, odd
    ref = (txt.clone(), vec.clone(), noise.clone(), cond.clone())
    if rank != 0:  # e.g. each rank's own VAE sample: only rank 0's may be stepped
        txt, vec, noise, cond = (torch.zeros_like(t) for t in (txt, vec, noise, cond))
    out = fdist.broadcast_request(txt, vec, noise, src=0, extra=cond)
    ok = len(out) == 4 and all(torch.equal(a, b) and a.shape == b.shape for a, b in zip(out, ref))
    # without `extra`: today's three tensors
    out3 = fdist.broadcast_request(*(ref[:3] if rank == 0 else (torch.zeros_like(t) for t in ref[:3])), src=0)
    ok = ok and len(out3) == 3 and all(torch.equal(a, b) for a, b in zip(out3, ref[:3]))
    q.put((rank, bool(ok)))
    td.barrier()
    td.destroy_process_group()


def test_broadcast_request_carries_the_reference_latents_over_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_broadcast_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res == [(0, True), (1, True)], res


def test_model_refuses_half_a_reference():
    from modules.flux_model import Flux

    img, ids = torch.zeros(1, 4, 64), torch.zeros(1, 4, 3)
    with pytest.raises(ValueError):
        Flux._with_reference(img, ids, torch.zeros(1, 3, 64), None)
    with pytest.raises(ValueError):
        Flux._with_reference(img, ids, torch.zeros(1, 3, 32), torch.zeros(1, 3, 3))
    s, i, Lc = Flux._with_reference(img, ids, torch.ones(1, 3, 64), torch.ones(1, 3, 3))
    assert Lc == 3 and s.shape == (1, 7, 64) and i.shape == (1, 7, 3) and (s[:, 4:] == 1).all() and (i[:, 4:] == 1).all()
    assert Flux._with_reference(img, ids, None, None) == (img, ids, 0)
