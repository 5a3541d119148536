"""FLUX IP-Adapter without a GPU: the error gate of tests/ip_adapter_ref.py (it admits a PyTorch evaluation of the term on every kernel case and
rejects six wrong terms), the XLabs-format loader, the CLIP preprocessing against transformers, and the refusals and plumbing of generate()
and /generate."""
import io

import numpy as np
import pytest
import torch

import ip_adapter_ref as ir


# ---- 1. the gate --------------------------------------------------------------------------------------------------------------------------
def test_gate_admits_torch_sdpa_on_every_kernel_case():
    worst = 0.0
    for rows, heads, nk, B in ir.KERNEL_CASES:
        q, w, k, v = ir.term_inputs(rows, heads, nk, B, seed=1)
        ref, A, E = ir.term_ref64(q, w, k, v)
        n_bad, r = ir.gate_violations(ir.term_sdpa_bf16(q, w, k, v), ref, A, E)
        worst = max(worst, r)
        assert n_bad == 0, f"rows {rows} heads {heads} nk {nk} B {B}: {n_bad} elements of torch's bf16 SDPA beyond the gate (worst {r:.3f})"
    print(f"torch bf16 SDPA: worst err / bound over {len(ir.KERNEL_CASES)} cases {worst:.3f}")


def _flat_inputs(rows, heads, nk, B, seed):
    """small keys (E ~ 0.3: the (1 + 2E) slack of the gate is small) and positive values (|ref| = A): the family on which a small
    multiplicative error of the output is visible to the gate"""
    q, w, k, v = ir.term_inputs(rows, heads, nk, B, seed)
    return q, w, (k.float() * 0.03).bfloat16(), v.float().abs().bfloat16()


def test_gate_rejects_wrong_terms():
    rows, heads, nk, B = 64, 3, 5, 2
    q, w, k, v = ir.term_inputs(rows, heads, nk, B, seed=2, nk_alloc=nk + 1)
    ref, A, E = ir.term_ref64(q, w, k, v, nk)
    good = ir.term_ref64(q, w, k, v, nk)[0].bfloat16()
    assert ir.gate_violations(good, ref, A, E)[0] == 0
    HD = heads * 128
    wrong = {
        "a dropped key": ir.term_ref64(q, w, k, v, nk - 1)[0],
        "an admitted key at index Nk": ir.term_ref64(q, w, k, v, nk + 1)[0],
        "a missing 128^-1/2": ir.term_ref64(q, w, k, v, nk, scale_logits=False)[0],
        "a missing q-norm scale": ir.term_ref64(q, w, k, v, nk, use_norm_scale=False)[0],
        "exchanged heads": ir.term_ref64(q, w, k, v, nk)[0].reshape(B, rows, heads, 128)[:, :, [1, 0, 2]].reshape(B, rows, HD),
    }
    for what, t in wrong.items():
        n_bad, r = ir.gate_violations(t.bfloat16(), ref, A, E)
        print(f"{what}: {n_bad} elements beyond the gate, worst err / bound {r:.2f}")
        assert n_bad > 0, f"the gate admits {what}"
    # a 2 % scale error is below the (1 + 2E) slack on unit-normal keys (E ~ 9); on small keys and positive values the gate sees it
    q, w, k, v = _flat_inputs(rows, heads, nk, B, seed=3)
    ref, A, E = ir.term_ref64(q, w, k, v)
    assert E.max() < 1.0
    assert ir.gate_violations(ref.bfloat16(), ref, A, E)[0] == 0
    assert ir.gate_violations(ir.term_sdpa_bf16(q, w, k, v), ref, A, E)[0] == 0
    n_bad, r = ir.gate_violations((ref * 1.02).bfloat16(), ref, A, E)
    print(f"a 2 % scale error: {n_bad} elements beyond the gate, worst err / bound {r:.2f}")
    assert n_bad > 0, "the gate admits a 2 % scale error"


def test_scale_table():
    from modules.ip_adapter import scale_table

    assert torch.equal(scale_table(0.7, 3, 2), torch.full((2, 3), 0.7))
    assert torch.equal(scale_table([0.1, 0.2, 0.3], 3, 2), torch.tensor([[0.1, 0.2, 0.3]] * 2))
    t = torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    assert torch.equal(scale_table(t, 3, 2), t) and torch.equal(scale_table(t[:1], 3, 2), t[:1].expand(2, 3))
    for bad in ([0.1, 0.2], [0.1] * 4, [], torch.ones(3, 3), torch.ones(2, 2), float("nan"), [1.0, float("inf"), 1.0]):
        with pytest.raises(ValueError, match="ip_adapter_scale"):
            scale_table(bad, 3, 2)


# ---- 2. the loader ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,depth,hidden", [(4, 3, 256), (16, 2, 128)])
def test_loader_infers_tokens_and_depth(tmp_path, T, depth, hidden):
    from safetensors.torch import save_file

    from fluxmi import synth
    from modules.ip_adapter import IPAdapter, check_state_dict, read_ip_adapter

    sd = synth.make_ip_adapter_state_dict(hidden, depth, T, seed=T)
    assert check_state_dict(sd) == (depth, T, hidden)
    path = str(tmp_path / "ip_adapter.safetensors")
    save_file({k: v.contiguous() for k, v in sd.items()}, path)
    m = read_ip_adapter(path)
    assert isinstance(m, IPAdapter) and (m.depth, m.num_tokens, m.hidden) == (depth, T, hidden) and m.clip is None
    assert torch.equal(m.ip_adapter_proj_model.proj.weight.bfloat16(), sd["ip_adapter_proj_model.proj.weight"])
    for i in range(depth):
        pre = f"double_blocks.{i}.processor.ip_adapter_double_stream_"
        assert torch.equal(m.k_proj[i].weight.bfloat16(), sd[pre + "k_proj.weight"]) and torch.equal(m.v_proj[i].bias.bfloat16(), sd[pre + "v_proj.bias"])
    with pytest.raises(RuntimeError, match="clip_vision_path"):
        m.embed(np.zeros((8, 8, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="not both"):
        m.call()


def test_loader_refuses_by_name():
    from fluxmi import synth
    from modules.ip_adapter import check_state_dict

    sd = synth.make_ip_adapter_state_dict(256, 3, 4)
    k1 = "double_blocks.1.processor.ip_adapter_double_stream_v_proj.bias"
    with pytest.raises(ValueError, match=k1.replace(".", r"\.")):
        check_state_dict({k: v for k, v in sd.items() if k != k1})
    with pytest.raises(ValueError, match=r"ip_adapter_proj_model\.norm\.weight"):
        check_state_dict({k: v for k, v in sd.items() if k != "ip_adapter_proj_model.norm.weight"})
    k2 = "double_blocks.2.processor.ip_adapter_double_stream_k_proj.weight"
    with pytest.raises(ValueError, match=k2.replace(".", r"\.") + r".*\[256, 4096\]"):
        check_state_dict({**sd, k2: sd[k2][:, :100]})
    with pytest.raises(ValueError, match=r"proj\.weight.*T \* 4096"):
        check_state_dict({**sd, "ip_adapter_proj_model.proj.weight": sd["ip_adapter_proj_model.proj.weight"][:5000]})
    with pytest.raises(ValueError, match=r"proj\.bias"):
        check_state_dict({**sd, "ip_adapter_proj_model.proj.bias": sd["ip_adapter_proj_model.proj.bias"][:4096]})
    with pytest.raises(ValueError, match="at most 64"):
        check_state_dict({**sd, "ip_adapter_proj_model.proj.weight": torch.zeros(65 * 4096, 768, dtype=torch.bfloat16)})
    # a diffusers-style file (FluxPipeline.load_ip_adapter's converted names) and an unrelated file
    diff = {"image_proj.proj.weight": sd["ip_adapter_proj_model.proj.weight"], "ip_adapter.0.to_k_ip.weight": sd[k2]}
    with pytest.raises(ValueError, match="diffusers-format"):
        check_state_dict(diff)
    with pytest.raises(ValueError, match="unknown key single_blocks"):
        check_state_dict({**sd, "single_blocks.0.processor.ip_adapter_single_stream_k_proj.weight": sd[k2]})
    with pytest.raises(ValueError, match="not an XLabs flux-ip-adapter file"):
        check_state_dict({"redux_up.weight": torch.zeros(4, 4)})


def test_load_ip_adapter_needs_both_local_paths(tmp_path):
    import util
    from safetensors.torch import save_file

    from fluxmi import synth

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    assert cfg.ip_adapter_path is None and cfg.clip_vision_path is None and util.load_ip_adapter(cfg) is None
    path = str(tmp_path / "ip.safetensors")
    save_file(synth.make_ip_adapter_state_dict(128, 1, 4), path)
    cfg.ip_adapter_path = path
    assert util.load_ip_adapter(cfg) is None                       # no tower: nothing is fetched by name
    cfg.clip_vision_path = "openai/clip-vit-large-patch14"
    assert util.load_ip_adapter(cfg) is None
    shipped = util.load_config_from_path(str(__import__("pathlib").Path(util.__file__).parent / "configs" / "config-dev-ip-adapter-mi355x.json"))
    assert shipped.ip_adapter_path and shipped.clip_vision_path and util.load_ip_adapter(shipped) is None


# ---- 3. preprocessing -------------------------------------------------------------------------------------------------------------------------
def test_clip_preprocess_is_transformers_bit_for_bit():
    from PIL import Image
    from transformers import CLIPImageProcessor

    from modules.ip_adapter import clip_preprocess

    proc = CLIPImageProcessor()  # the defaults: openai/clip-vit-large-patch14's preprocessor_config.json
    assert proc.size == {"shortest_edge": 224} and proc.crop_size == {"height": 224, "width": 224} and proc.resample == 3
    rng = np.random.default_rng(0)
    for h, w in ((301, 227), (225, 399), (224, 224), (97, 131), (640, 223)):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        a[: h // 2] //= 2
        want = torch.from_numpy(proc(images=Image.fromarray(a), return_tensors="np")["pixel_values"])
        got = clip_preprocess(a)
        assert got.shape == (1, 3, 224, 224) and got.dtype == torch.float32
        assert torch.equal(got, want), f"{h}x{w}: max |d| {float((got - want).abs().max()):.3e}"
    grey = rng.integers(0, 256, (240, 250), dtype=np.uint8)  # a one-channel image is converted to RGB first
    assert torch.equal(clip_preprocess(grey), torch.from_numpy(proc(images=Image.fromarray(grey).convert("RGB"), return_tensors="np")["pixel_values"]))


# ---- 4. generate() and /generate ------------------------------------------------------------------------------------------------------------------
class _FakeModel:
    """stands in for Flux in FluxPipeline: records the denoise calls"""

    def __init__(self, params):
        self.params, self.calls = params, []
        self.in_channels = self.out_channels = params.in_channels
        self.hidden_size, self.double_blocks = params.hidden_size, [None] * params.depth

    def denoise(self, img, img_ids, txt, txt_ids, y, timesteps, **kw):
        self.calls.append(dict(kw, ts=list(timesteps)))
        return img


class _FakeAdapter:
    """stands in for modules.ip_adapter.IPAdapter: K / V that tell which embeds they came from"""
    clip = None

    def __init__(self, depth, hidden, T=4):
        self.depth, self.hidden, self.num_tokens, self.embedded = depth, hidden, T, []

    def embed(self, images):
        images = images if isinstance(images, (list, tuple)) else [images]
        self.embedded.append(images)
        return torch.stack([torch.full((768,), float(np.asarray(im).mean())) for im in images])

    def kv(self, emb):
        n = emb.shape[0]
        k = emb[:, :1].repeat_interleave(self.num_tokens, 0)[None, None].expand(self.depth, 1, n * self.num_tokens, self.hidden)
        return k.clone(), -k.clone()


def make_pipe(adapter, depth=2):
    import util
    from flux_pipeline import FluxPipeline

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    p = cfg.params
    p.hidden_size, p.num_heads, p.depth, p.depth_single_blocks, p.context_in_dim, p.vec_in_dim = 256, 2, depth, 1, 128, 64
    pipe = FluxPipeline.__new__(FluxPipeline)
    pipe.name, pipe.debug, pipe.dtype, pipe.ae_dtype = "flux-dev", False, torch.bfloat16, torch.bfloat16
    pipe.device_flux = pipe.device_ae = pipe.device_clip = pipe.device_t5 = torch.device("cpu")
    pipe.model, pipe.ae, pipe.clip, pipe.t5, pipe.rng = _FakeModel(cfg.params), None, None, None, torch.Generator(device="cpu")
    pipe.redux, pipe.controlnet, pipe.ip_adapter, pipe.config = None, None, adapter, cfg
    return pipe


def test_generate_refusals_and_plumbing():
    g = torch.Generator().manual_seed(1)
    prompt = {"txt": 0.1 * torch.randn(1, 32, 128, generator=g), "vec": torch.randn(1, 64, generator=g)}
    KW = dict(width=64, height=64, num_steps=4, seed=7, silent=True, output_type="latent")
    emb = torch.randn(1, 768, generator=g)
    white = np.full((30, 40, 3), 255, dtype=np.uint8)
    with pytest.raises(ValueError, match="ip_adapter_path"):
        make_pipe(None).generate(prompt, ip_adapter_image_embeds=emb, **KW)
    pipe = make_pipe(_FakeAdapter(2, 256))
    with pytest.raises(ValueError, match="regions"):
        pipe.generate(prompt, ip_adapter_image_embeds=emb, regions=[{"prompt": prompt, "box": (0, 0, 1, 1)}], **KW)
    with pytest.raises(ValueError, match="cache_threshold"):
        pipe.generate(prompt, ip_adapter_image_embeds=emb, cache_threshold=0.1, **KW)
    with pytest.raises(ValueError, match="not both"):
        pipe.generate(prompt, ip_adapter_image_embeds=emb, ip_adapter_image=white, **KW)
    with pytest.raises(ValueError, match="ip_adapter_scale"):
        pipe.generate(prompt, ip_adapter_image_embeds=emb, ip_adapter_scale=[0.5, 0.5, 0.5], **KW)  # 3 floats for 2 double blocks
    with pytest.raises(ValueError, match="ip_adapter_scale"):
        pipe.generate(prompt, ip_adapter_image_embeds=emb, negative_ip_adapter_scale=[0.5], **KW)
    with pytest.raises(ValueError, match="negative_ip_adapter_image goes with"):
        pipe.generate(prompt, negative_ip_adapter_image=white, **KW)
    with pytest.raises(ValueError, match="double blocks"):
        make_pipe(_FakeAdapter(3, 256)).generate(prompt, ip_adapter_image_embeds=emb, **KW)
    assert not pipe.model.calls
    # without the arguments the request is today's: no ip_adapter argument reaches the model
    pipe.generate(prompt, **KW)
    assert len(pipe.model.calls) == 1 and "ip_adapter" not in pipe.model.calls[0]
    pipe.model.calls.clear()
    # embeds skip the tower; the scale list reaches the call as a [1, depth] table
    pipe.generate(prompt, ip_adapter_image_embeds=emb, ip_adapter_scale=[0.25, 0.75], **KW)
    (c,) = pipe.model.calls
    ip = c["ip_adapter"]
    assert not pipe.ip_adapter.embedded and ip.k_ip.shape == (2, 1, 4, 256) and torch.equal(ip.scale, torch.tensor([[0.25, 0.75]]))
    assert torch.equal(ip.k_ip[0, 0, 0], emb[0, :1].expand(256))
    pipe.model.calls.clear()
    # two images: Nk = 2 T, in list order; a guided request: the negative branch's black images (as many), its own scale, guided steps only
    black = np.zeros((30, 40, 3), dtype=np.uint8)
    neg = {"txt": 0.1 * torch.randn(1, 32, 128, generator=g), "vec": torch.randn(1, 64, generator=g)}
    pipe.generate(prompt, ip_adapter_image=[white, white // 2], ip_adapter_scale=0.5, negative_prompt=neg, true_cfg_scale=3.0,
                  true_cfg_interval=(0.0, 0.5), negative_ip_adapter_scale=0.125, **KW)
    guided, plain = pipe.model.calls
    assert len(guided["ts"]) == 3 and len(plain["ts"]) == 3 and "neg_txt" in guided and "neg_txt" not in plain
    assert plain["ip_adapter"].k_ip.shape == (2, 1, 8, 256) and guided["ip_adapter"].k_ip.shape == (2, 2, 8, 256)
    assert [len(e) for e in pipe.ip_adapter.embedded] == [2, 2] and all(np.asarray(im).max() == 0 for im in pipe.ip_adapter.embedded[1])
    assert float(guided["ip_adapter"].k_ip[0, 0, 0, 0]) == 255.0 and float(guided["ip_adapter"].k_ip[0, 0, 4, 0]) == 127.0
    assert float(guided["ip_adapter"].k_ip[0, 1].abs().max()) == 0.0
    assert torch.equal(guided["ip_adapter"].scale, torch.tensor([[0.5, 0.5], [0.125, 0.125]])) and torch.equal(plain["ip_adapter"].scale, torch.tensor([[0.5, 0.5]]))
    with pytest.raises(ValueError, match="the same number of image tokens"):
        pipe.generate(prompt, ip_adapter_image=[white, white], negative_prompt=neg, true_cfg_scale=3.0, negative_ip_adapter_image=black, **KW)


def test_model_level_refusals():
    """Flux.forward / Flux.denoise refuse before any device work"""
    import util
    from modules.ip_adapter import IPAdapterCall

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    p = cfg.params
    p.hidden_size, p.num_heads, p.depth, p.depth_single_blocks, p.context_in_dim, p.vec_in_dim = 256, 2, 2, 1, 128, 64
    from fluxmi import synth

    model = util.load_flow_model(cfg, synth.make_state_dict(p, seed=0))
    inp = synth.make_inputs(p, 64, 64, 32, batch=2, seed=0)
    args = (inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], inp["y"], [1.0, 0.5])
    ok = IPAdapterCall(torch.zeros(2, 1, 4, 256), torch.zeros(2, 1, 4, 256), 1.0)
    with pytest.raises(ValueError, match="attn_groups"):
        model.denoise(*args, ip_adapter=ok, attn_groups=torch.zeros(1, 48, dtype=torch.int32))
    with pytest.raises(ValueError, match="cache_threshold"):
        model.denoise(*args, ip_adapter=ok, cache_threshold=0.1)
    with pytest.raises(ValueError, match="Nk = 65"):
        model.denoise(*args, ip_adapter=IPAdapterCall(torch.zeros(2, 1, 65, 256), torch.zeros(2, 1, 65, 256)))
    with pytest.raises(ValueError, match="expected two tensors"):
        model.denoise(*args, ip_adapter=IPAdapterCall(torch.zeros(3, 1, 4, 256), torch.zeros(3, 1, 4, 256)))  # depth 3 on a model of 2
    with pytest.raises(ValueError, match="expected two tensors"):
        model.denoise(*args, ip_adapter=IPAdapterCall(torch.zeros(2, 3, 4, 256), torch.zeros(2, 3, 4, 256)))  # 3 samples on a batch of 2
    with pytest.raises(ValueError, match="ip_adapter_scale"):
        model.denoise(*args, ip_adapter=IPAdapterCall(ok.k_ip, ok.v_ip, [1.0, 1.0, 1.0]))


def test_api_fields_and_http():
    """the adapter's fields reach generate() only when set; a request without them produces exactly today's keyword arguments"""
    from fastapi.testclient import TestClient

    import api

    f = api.GenerateArgs.model_fields
    for k in ("ip_adapter_image", "ip_adapter_image_embeds", "ip_adapter_scale", "negative_ip_adapter_image", "negative_ip_adapter_scale"):
        assert k in f and f[k].default is None
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
    r = c.post("/generate", json={**base, "ip_adapter_image": ["a.png", "b.png"], "ip_adapter_scale": [0.5] * 19, "negative_ip_adapter_scale": 0.2})
    assert r.status_code == 200 and r.content.startswith(b"\xff\xd8")
    assert calls[-1]["ip_adapter_image"] == ["a.png", "b.png"] and calls[-1]["ip_adapter_scale"] == [0.5] * 19
    assert calls[-1]["negative_ip_adapter_scale"] == 0.2 and "negative_ip_adapter_image" not in calls[-1] and "ip_adapter_image_embeds" not in calls[-1]
    assert c.post("/generate", json={**base, "ip_adapter_image": "a.png", "ip_adapter_scale": 0.8}).status_code == 200
    assert calls[-1]["ip_adapter_image"] == "a.png" and calls[-1]["ip_adapter_scale"] == 0.8
    assert c.post("/generate", json={**base, "ip_adapter_image_embeds": [[0.5] * 768]}).status_code == 200
    e = calls[-1]["ip_adapter_image_embeds"]
    assert isinstance(e, torch.Tensor) and e.shape == (1, 768) and e.dtype == torch.float32 and "ip_adapter_image" not in calls[-1]
    assert c.post("/generate", json={**base, "ip_adapter_scale": "strong"}).status_code == 422
