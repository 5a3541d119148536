"""First-block step caching, host side: what FluxPipeline.generate / Flux.denoise refuse without a device, which denoise calls a cached
request turns into (the arguments are forwarded only when caching is on, every segment of a true_cfg_interval request gets them), the HTTP
fields, and the C ABI entries.  No GPU."""
import io
import re
import os

import pytest
import torch

from test_cfg_cpu import KW, embeddings, make_pipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class CachingStubFlow:
    """records every denoise call together with the cache arguments it was given"""

    def __init__(self):
        self.calls = []

    def denoise(self, img, img_ids, txt, txt_ids, vec, timesteps, guidance=3.5, use_graph=True, neg_txt=None, neg_y=None, cfg_scale=1.0, **kw):
        self.calls.append(dict(ts=list(timesteps), guided=neg_txt is not None, kw=kw))
        return (img.float() * 2 + len(timesteps)).to(img.dtype)


def test_generate_forwards_the_cache_arguments_only_when_caching_is_on():
    pos, neg = embeddings(1, 1), embeddings(1, 2)
    # off (absent, 0, 0.0 with a hit bound): the flow model sees exactly today's keyword arguments -- the strict stub of test_cfg_cpu takes no others
    plain = make_pipe().generate(pos, **KW)
    for extra in (dict(cache_threshold=0), dict(cache_threshold=0.0, cache_max_hits=3)):
        pipe = make_pipe()
        assert torch.equal(pipe.generate(pos, **extra, **KW), plain)
    pipe = make_pipe(CachingStubFlow())
    pipe.generate(pos, **KW)
    assert pipe.model.calls[-1]["kw"] == {}
    pipe.generate(pos, cache_threshold=0.125, **KW)
    assert pipe.model.calls[-1]["kw"] == dict(cache_threshold=0.125, cache_max_hits=0)
    pipe.generate(pos, cache_threshold="0.25", cache_max_hits=2, **KW)
    assert pipe.model.calls[-1]["kw"] == dict(cache_threshold=0.25, cache_max_hits=2)
    # every denoise call of a true_cfg_interval request gets them (each starts with an empty cache: the engine's rule, per call)
    pipe = make_pipe(CachingStubFlow())
    pipe.generate(pos, negative_prompt=neg, true_cfg_scale=3.5, true_cfg_interval=(0.25, 0.75), cache_threshold=0.5, cache_max_hits=1, **KW)
    assert [c["guided"] for c in pipe.model.calls] == [False, True, False]
    assert all(c["kw"] == dict(cache_threshold=0.5, cache_max_hits=1) for c in pipe.model.calls)


@pytest.mark.parametrize("bad", [dict(cache_threshold=-0.1), dict(cache_threshold=float("nan")), dict(cache_threshold=float("inf")),
                                 dict(cache_threshold="x"), dict(cache_threshold=None), dict(cache_threshold=0.1, cache_max_hits=-1),
                                 dict(cache_threshold=0.0, cache_max_hits=-2)])
def test_generate_refuses_bad_cache_arguments(bad):
    pipe = make_pipe()
    with pytest.raises(ValueError, match="cache_threshold|cache_max_hits"):
        pipe.generate(embeddings(1, 1), **bad, **KW)
    assert pipe.model.calls == [], "a refused request reached the flow model"


def test_denoise_validates_the_cache_arguments_before_any_device_work():
    import util
    from fluxmi import synth

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    p = cfg.params
    p.hidden_size, p.num_heads, p.depth, p.depth_single_blocks, p.context_in_dim, p.vec_in_dim = 256, 2, 1, 1, 128, 64
    model = util.load_flow_model(cfg, synth.make_state_dict(p, seed=0))
    img, ids = torch.zeros(1, 4, 64), torch.zeros(1, 4, 3)
    txt, tids, y = torch.zeros(1, 6, 128), torch.zeros(1, 6, 3), torch.zeros(1, 64)
    for bad in (dict(cache_threshold=-1.0), dict(cache_threshold=float("nan")), dict(cache_threshold=float("inf")), dict(cache_max_hits=-1)):
        with pytest.raises(ValueError, match="cache_threshold"):
            model.denoise(img, ids, txt, tids, y, [1.0, 0.5, 0.0], **bad)
    assert model._engine is None, "a refused request created the engine"
    ratios, hits = model.step_cache_log()
    assert ratios.numel() == 0 and hits == []


def test_c_abi_has_the_step_cache_entries_and_no_new_knob():
    from fluxmi import _lib

    for name in ("fluxmi_fb_snapshot", "fluxmi_fb_metric", "fluxmi_fb_commit", "fluxmi_fb_store", "fluxmi_fb_apply", "fluxmi_engine_set_step_cache",
                 "fluxmi_engine_step_cache_log", "fluxmi_engine_run_phase"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
    assert _lib.lib.fluxmi_abi_version() == 5
    # the threshold is request state, not a kernel-selection knob: fluxmi_tuning_t is what it was
    hdr = open(os.path.join(ROOT, "include", "fluxmi.h")).read()
    body = re.search(r"typedef struct fluxmi_tuning \{(.*?)\} fluxmi_tuning_t;", hdr, flags=re.S)
    assert body and "step_cache" not in body.group(1) and "fb_" not in body.group(1) and len(_lib.Tuning._fields_) == 20
    # refusals that need no device: NULL engine
    with pytest.raises(RuntimeError, match="NULL engine"):
        _lib.call("fluxmi_engine_set_step_cache", None, 0.1, 0)


def test_http_cache_fields():
    """`cache_threshold` / `cache_max_hits` reach generate() only when set; a request without them produces exactly today's keyword arguments."""
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
    assert c.post("/generate", json={**base, "cache_threshold": None, "cache_max_hits": None}).status_code == 200
    assert not {"cache_threshold", "cache_max_hits"} & set(calls[-1])
    r = c.post("/generate", json={**base, "cache_threshold": 0.08})
    assert r.status_code == 200 and r.content.startswith(b"\xff\xd8")
    assert calls[-1]["cache_threshold"] == 0.08 and "cache_max_hits" not in calls[-1]
    r = c.post("/generate", json={**base, "cache_threshold": 0.1, "cache_max_hits": 2, "negative_prompt": "", "true_cfg_scale": 2.0})
    assert r.status_code == 200 and calls[-1]["cache_max_hits"] == 2 and calls[-1]["cache_threshold"] == 0.1 and calls[-1]["negative_prompt"] == ""
    assert c.post("/generate", json={**base, "cache_threshold": "often"}).status_code == 422
    assert c.post("/generate", json={**base, "cache_max_hits": 1.5}).status_code == 422
