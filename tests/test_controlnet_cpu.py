"""FLUX ControlNet, the parts that need no GPU: the diffusers-name converter, the step-interval and block-index functions, self-checks of the
composed reference (tests/controlnet_ref.py), the host-only layer count and the Python-level refusals."""
import ctypes as C
import re

import pytest
import torch

import controlnet_ref as cr
import flux_oracle as fo


def tiny_config(depth=3, single=4):
    import util

    cfg = util.load_config(util.ModelVersion.flux_dev, flow_dtype="bfloat16")
    p = cfg.params
    p.hidden_size, p.num_heads, p.depth, p.depth_single_blocks, p.context_in_dim, p.vec_in_dim = 256, 2, depth, single, 128, 64
    return cfg


# ---- 1. converter ------------------------------------------------------------------------------------------------------------------------
def to_diffusers(sd, H):
    """BFL-style FluxControlNet names -> diffusers' FluxControlNetModel names (the inverse of what the converter does, written out here)"""
    top = {"img_in": "x_embedder", "txt_in": "context_embedder", "time_in.in_layer": "time_text_embed.timestep_embedder.linear_1",
           "time_in.out_layer": "time_text_embed.timestep_embedder.linear_2", "vector_in.in_layer": "time_text_embed.text_embedder.linear_1",
           "vector_in.out_layer": "time_text_embed.text_embedder.linear_2", "guidance_in.in_layer": "time_text_embed.guidance_embedder.linear_1",
           "guidance_in.out_layer": "time_text_embed.guidance_embedder.linear_2"}
    dbl = {"img_mod.lin": "norm1.linear", "txt_mod.lin": "norm1_context.linear", "img_attn.proj": "attn.to_out.0", "txt_attn.proj": "attn.to_add_out",
           "img_mlp.0": "ff.net.0.proj", "img_mlp.2": "ff.net.2", "txt_mlp.0": "ff_context.net.0.proj", "txt_mlp.2": "ff_context.net.2"}
    dnorm = {"img_attn.norm.query_norm.scale": "attn.norm_q.weight", "img_attn.norm.key_norm.scale": "attn.norm_k.weight",
             "txt_attn.norm.query_norm.scale": "attn.norm_added_q.weight", "txt_attn.norm.key_norm.scale": "attn.norm_added_k.weight"}
    out = {}
    for k, v in sd.items():
        stem, _, leaf = k.rpartition(".")
        m = re.match(r"(double_blocks|single_blocks)\.(\d+)\.(.+)$", k)
        if k.startswith("controlnet_"):
            out[k] = v
        elif stem in top:
            out[f"{top[stem]}.{leaf}"] = v
        elif m and m.group(1) == "double_blocks":
            i, rest = m.group(2), m.group(3)
            pre = f"transformer_blocks.{i}."
            rstem = rest.rpartition(".")[0]
            if rest in dnorm:
                out[pre + dnorm[rest]] = v
            elif rstem in dbl:
                out[f"{pre}{dbl[rstem]}.{leaf}"] = v
            elif rstem in ("img_attn.qkv", "txt_attn.qkv"):
                names = ("to_q", "to_k", "to_v") if rstem.startswith("img") else ("add_q_proj", "add_k_proj", "add_v_proj")
                for n, part in zip(names, v.chunk(3, 0)):
                    out[f"{pre}attn.{n}.{leaf}"] = part.clone()
            else:
                raise AssertionError(k)
        elif m:
            i, rest = m.group(2), m.group(3)
            pre = f"single_transformer_blocks.{i}."
            rstem = rest.rpartition(".")[0]
            if rest == "norm.query_norm.scale":
                out[pre + "attn.norm_q.weight"] = v
            elif rest == "norm.key_norm.scale":
                out[pre + "attn.norm_k.weight"] = v
            elif rstem == "modulation.lin":
                out[f"{pre}norm.linear.{leaf}"] = v
            elif rstem == "linear2":
                out[f"{pre}proj_out.{leaf}"] = v
            elif rstem == "linear1":
                parts = torch.split(v, [H, H, H, v.shape[0] - 3 * H], 0)
                for n, part in zip(("attn.to_q", "attn.to_k", "attn.to_v", "proj_mlp"), parts):
                    out[f"{pre}{n}.{leaf}"] = part.clone()
            else:
                raise AssertionError(k)
        else:
            raise AssertionError(k)
    return out


@pytest.mark.parametrize("nd,ns,num_mode,guid", [(2, 2, 0, True), (2, 1, 3, False), (3, 0, 0, True)])
def test_converter_inverts_the_diffusers_names(nd, ns, num_mode, guid):
    from fluxmi import synth
    from modules import controlnet as cn

    cfg = tiny_config()
    sd = synth.make_controlnet_state_dict(cfg.params, nd, ns, num_mode, seed=1, guidance_embed=guid)
    dsd = to_diffusers(sd, cfg.params.hidden_size)
    assert "transformer_blocks.0.attn.to_q.weight" in dsd and "x_embedder.weight" in dsd and not any(k.startswith("double_blocks") for k in dsd)
    info = cn.inspect_diffusers_controlnet(dsd)
    assert (info["num_double"], info["num_single"], info["num_mode"], info["guidance_embed"]) == (nd, ns, num_mode, guid)
    assert info["hidden_size"] == 256 and info["in_channels"] == 64
    keys_before = set(dsd)
    back = cn.convert_diffusers_controlnet_checkpoint(dsd)
    assert set(dsd) == keys_before, "the converter consumed its input"
    assert set(back) == set(sd)
    for k in sd:
        assert back[k].dtype == sd[k].dtype and torch.equal(back[k], sd[k]), k
    # both spellings load into the module, whose state dict is the BFL-named one
    for src in (dsd, sd):
        net = cn.FluxControlNet.from_state_dict(cfg, src)
        assert set(net.state_dict()) == set(sd)
        assert net.params.depth == nd and net.params.depth_single_blocks == ns and net.num_mode == num_mode and net.params.guidance_embed == guid
        assert all(torch.equal(net.state_dict()[k], sd[k]) for k in sd)
        assert net.final_layer is None and len(net.linear_modules()) == 6 + (2 if guid else 0) + 10 * nd + 3 * ns + 1 + nd + ns


def test_converter_refuses_xlabs_and_unknown_checkpoints():
    from fluxmi import synth
    from modules import controlnet as cn

    cfg = tiny_config()
    dsd = to_diffusers(synth.make_controlnet_state_dict(cfg.params, 2, 0, seed=1), 256)
    with pytest.raises(ValueError, match="input_hint_block"):
        cn.convert_diffusers_controlnet_checkpoint({**dsd, "input_hint_block.0.weight": torch.zeros(16, 3, 3, 3)})
    with pytest.raises(ValueError, match="input_hint_block"):
        cn.FluxControlNet.from_state_dict(cfg, {"input_hint_block.0.weight": torch.zeros(16, 3, 3, 3), "double_blocks.0.img_mod.lin.weight": torch.zeros(4, 4)})
    with pytest.raises(ValueError, match="controlnet_x_embedder"):
        cn.inspect_diffusers_controlnet({"x_embedder.weight": torch.zeros(4, 4)})
    with pytest.raises(ValueError, match="does not know"):
        cn.convert_diffusers_controlnet_checkpoint({**dsd, "some_other.weight": torch.zeros(2, 2)})
    less = {k: v for k, v in dsd.items() if k != "transformer_blocks.1.attn.to_k.weight"}
    with pytest.raises(KeyError, match="to_k"):
        cn.convert_diffusers_controlnet_checkpoint(less)


def test_load_controlnet_needs_a_local_path(tmp_path):
    import util
    from fluxmi import synth
    from safetensors.torch import save_file

    cfg = tiny_config()
    assert util.load_controlnet(cfg) is None
    cfg.controlnet_path = "InstantX/FLUX.1-dev-Controlnet-Canny"  # a hub id, not a local path: nothing is downloaded
    assert util.load_controlnet(cfg) is None
    sd = to_diffusers(synth.make_controlnet_state_dict(cfg.params, 2, 1, 2, seed=3), 256)
    d = tmp_path / "net"
    d.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(d / "diffusion_pytorch_model.safetensors"))
    for path in (str(d), str(d / "diffusion_pytorch_model.safetensors")):
        cfg.controlnet_path = path
        net = util.load_controlnet(cfg)
        assert net is not None and net.num_mode == 2 and net.params.depth == 2 and net.params.depth_single_blocks == 1


# ---- 2. step interval, block index ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start,end,want", [(0.0, 1.0, "1111"), (0.0, 0.5, "1100"), (0.25, 0.75, "0110"), (0.0, 0.0, "0000")])
def test_control_steps(start, end, want):
    from modules.controlnet import control_steps

    assert "".join("1" if k else "0" for k in control_steps(4, start, end)) == want


def test_block_index_map():
    from modules.controlnet import residual_index

    assert "".join(str(residual_index(i, 19, 5)) for i in range(19)) == "0000111122223333444"
    assert max(residual_index(i, 38, 10) for i in range(38)) == 9
    assert max(residual_index(i, 19, 6) for i in range(19)) == 4
    for n, r in ((19, 5), (38, 10), (19, 6), (3, 2), (4, 2), (4, 1), (4, 4)):
        assert [residual_index(i, n, r) for i in range(n)] == [cr.block_index(i, n, r) for i in range(n)]
        assert max(residual_index(i, n, r) for i in range(n)) < r


# ---- 3. the composed reference -------------------------------------------------------------------------------------------------------------
def ref_setup(nd=2, ns=2, num_mode=0, seed=0):
    from fluxmi import synth

    cfg = tiny_config()
    params = fo.FluxParams(**cfg.params.model_dump())
    sd = synth.make_state_dict(cfg.params, seed=seed)
    net_sd = synth.make_controlnet_state_dict(cfg.params, nd, ns, num_mode, seed=seed)
    inp = synth.make_inputs(cfg.params, 64, 64, 32, batch=2, seed=3, real_tokens=8)
    g = torch.Generator().manual_seed(77)
    inp["cond"] = torch.randn(2, inp["img"].shape[1], 64, generator=g).to(torch.bfloat16)
    return cfg, params, sd, net_sd, inp


def test_reference_with_zeroed_projections_is_the_plain_oracle():
    cfg, params, sd, net_sd, inp = ref_setup(num_mode=2)
    for k in net_sd:
        if k.startswith(("controlnet_blocks", "controlnet_single_blocks")):
            net_sd[k] = torch.zeros_like(net_sd[k])
    main = fo.FluxOracle(sd, params)
    net = cr.make_net_oracle(net_sd, params)
    t = torch.full((2,), 0.75, dtype=torch.bfloat16)
    g = torch.full((2,), 3.5, dtype=torch.bfloat16)
    args = (inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], t, inp["y"], g)
    plain = main.forward(*args)
    assert torch.equal(cr.forward(main, None, *args), plain)
    assert torch.equal(cr.forward(main, net, *args, cond=inp["cond"], mode=1, scale=0.7), plain)


@pytest.mark.parametrize("nd,ns,num_mode", [(2, 2, 0), (2, 1, 3), (2, 0, 0)])
def test_reference_synthetic_net_moves_the_output(nd, ns, num_mode):
    """the GPU parity gates are 1e-2 (bf16) and 6e-2 (fp8): the synthetic projections must move the oracle's own output by >= 10 x the loosest"""
    cfg, params, sd, net_sd, inp = ref_setup(nd, ns, num_mode)
    main = fo.FluxOracle(sd, params)
    net = cr.make_net_oracle(net_sd, params)
    assert net.n_f8() == 0 and net.p.depth == nd and net.p.depth_single_blocks == ns
    netq = cr.make_net_oracle(net_sd, params, quantize=dict(modulation=True, embedders=True))
    assert not any(isinstance(m, fo.F8LinearState) for n, m in netq.lin.items() if n.startswith("controlnet_")) and netq.n_f8() > 0
    t = torch.full((2,), 0.75, dtype=torch.bfloat16)
    g = torch.full((2,), 3.5, dtype=torch.bfloat16)
    args = (inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], t, inp["y"], g)
    plain = main.forward(*args).float()
    mode = 1 if num_mode else None
    for s in (0.4, 1.0):
        on = cr.forward(main, net, *args, cond=inp["cond"], mode=mode, scale=s).float()
        d = ((on - plain).norm() / plain.norm()).item()
        print(f"net {nd}+{ns} scale {s}: ControlNet on vs off rel-L2 {d:.3f}")
        assert d >= 0.1, f"scale {s}: on vs off rel-L2 {d:.3e}"
    if num_mode:
        a = cr.forward(main, net, *args, cond=inp["cond"], mode=0).float()
        b = cr.forward(main, net, *args, cond=inp["cond"], mode=2).float()
        assert ((a - b).norm() / b.norm()).item() > 1e-2, "the control mode does not reach the output"


# ---- 4. host-only layer count, Python-level refusals ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd,ns,guid", [(5, 10, 1), (5, 0, 0), (2, 1, 1)])
def test_controlnet_num_linears(nd, ns, guid):
    from fluxmi import _lib

    d = _lib.ModelDesc()
    d.hidden, d.heads, d.mlp_hidden, d.depth, d.depth_single, d.in_channels, d.vec_in, d.ctx_in, d.guidance_embed = 3072, 24, 12288, nd, ns, 64, 768, 4096, guid
    trunk = _lib.lib.fluxmi_engine_num_linears(C.byref(d))
    assert trunk == 6 + 2 * guid + 10 * nd + 3 * ns + 2
    assert _lib.lib.fluxmi_controlnet_num_linears(C.byref(d)) == trunk - 2 + 1 + nd + ns
    assert _lib.lib.fluxmi_controlnet_num_linears(None) == -1


def test_python_level_refusals():
    import util
    from fluxmi import synth
    from modules.controlnet import ControlNetCall, FluxControlNet

    cfg = tiny_config(1, 1)
    model = util.load_flow_model(cfg, synth.make_state_dict(cfg.params, seed=0))
    net = FluxControlNet.from_state_dict(cfg, synth.make_controlnet_state_dict(cfg.params, 1, 1, seed=0))
    union = FluxControlNet.from_state_dict(cfg, synth.make_controlnet_state_dict(cfg.params, 1, 0, 3, seed=0))
    B, Li, Lt = 2, 4, 6
    img, ids = torch.zeros(B, Li, 64), torch.zeros(B, Li, 3)
    txt, tids, y = torch.zeros(B, Lt, 128), torch.zeros(B, Lt, 3), torch.zeros(B, 64)
    cond = torch.zeros(B, Li, 64)
    ts = [1.0, 0.5, 0.0]
    call = lambda c, **kw: model.denoise(img, ids, txt, tids, y, ts, controlnet=c, **kw)
    ok = ControlNetCall(net, cond)
    with pytest.raises(ValueError, match="attn_groups"):
        call(ok, attn_groups=torch.zeros(1, Lt + Li, dtype=torch.int32))
    with pytest.raises(ValueError, match="cache_threshold"):
        call(ok, cache_threshold=0.1)
    with pytest.raises(ValueError, match="Kontext"):
        call(ok, img_cond_seq=torch.zeros(B, 2, 64), img_cond_seq_ids=torch.zeros(B, 2, 3))
    with pytest.raises(ValueError, match="Union net needs control_mode"):
        call(ControlNetCall(union, cond))
    with pytest.raises(ValueError, match="Union net needs control_mode"):
        call(ControlNetCall(union, cond, 1.0, 3))
    with pytest.raises(ValueError, match="without a mode embedding"):
        call(ControlNetCall(net, cond, 1.0, 0))
    with pytest.raises(ValueError, match="cond"):
        call(ControlNetCall(net, cond[:, :3]))
    with pytest.raises(ValueError, match="cond"):
        call(ControlNetCall(net, torch.zeros(3, Li, 64)))
    with pytest.raises(ValueError, match="not finite"):
        call(ControlNetCall(net, cond, float("nan")))
    with pytest.raises(ValueError, match="attn_groups"):
        model(img, ids, txt, tids, torch.ones(B), y, torch.ones(B), controlnet=ok, attn_groups=torch.zeros(1, Lt + Li, dtype=torch.int32))
    # a Fill / Depth / Canny model takes none
    fcfg = tiny_config(1, 1)
    fcfg.params.in_channels, fcfg.params.out_channels = 128, 64
    fill = util.load_flow_model(fcfg, synth.make_state_dict(fcfg.params, seed=0))
    with pytest.raises(ValueError, match="Fill / Depth / Canny"):
        fill.denoise(img, ids, txt, tids, y, ts, img_cond=torch.zeros(B, Li, 64), controlnet=ok)
    with pytest.raises(ValueError, match="Fill / Depth / Canny"):
        FluxControlNet(fcfg, 1, 0)
    # another geometry
    wcfg = tiny_config(1, 1)
    wcfg.params.hidden_size, wcfg.params.num_heads = 384, 3
    wide = FluxControlNet.from_state_dict(wcfg, synth.make_controlnet_state_dict(wcfg.params, 1, 0, seed=0))
    with pytest.raises(ValueError, match="differ"):
        call(ControlNetCall(wide, cond))
    with pytest.raises(RuntimeError, match="attached"):
        net(img, ids, txt, tids, torch.ones(B), y)
    # a net with a guidance embedder on a main model without one
    scfg = tiny_config(1, 1)
    scfg.params.guidance_embed = False
    schnell = util.load_flow_model(scfg, synth.make_state_dict(scfg.params, seed=0))
    with pytest.raises(ValueError, match="guidance embedder"):
        schnell.denoise(img, ids, txt, tids, y, ts, controlnet=ok)


class _FakeModel:
    """stands in for Flux in FluxPipeline: records the denoise calls"""
    params = None

    def __init__(self, params):
        self.params, self.calls = params, []
        self.in_channels = self.out_channels = params.in_channels

    def denoise(self, img, img_ids, txt, txt_ids, y, timesteps, **kw):
        self.calls.append(dict(kw, ts=list(timesteps)))
        return img


def make_pipe(net):
    from flux_pipeline import FluxPipeline

    cfg = tiny_config(1, 1)
    pipe = FluxPipeline.__new__(FluxPipeline)
    pipe.name, pipe.debug, pipe.dtype, pipe.ae_dtype = "flux-dev", False, torch.bfloat16, torch.bfloat16
    pipe.device_flux = pipe.device_ae = pipe.device_clip = pipe.device_t5 = torch.device("cpu")
    pipe.model, pipe.ae, pipe.clip, pipe.t5, pipe.rng = _FakeModel(cfg.params), None, None, None, torch.Generator(device="cpu")
    pipe.redux, pipe.controlnet, pipe.config = None, net, cfg
    return pipe


def test_pipeline_refusals_and_interval_slicing():
    from fluxmi import synth
    from modules.controlnet import FluxControlNet

    cfg = tiny_config(1, 1)
    net = FluxControlNet.from_state_dict(cfg, synth.make_controlnet_state_dict(cfg.params, 1, 0, seed=0))
    union = FluxControlNet.from_state_dict(cfg, synth.make_controlnet_state_dict(cfg.params, 1, 0, 3, seed=0))
    g = torch.Generator().manual_seed(1)
    prompt = {"txt": 0.1 * torch.randn(1, 32, 128, generator=g), "vec": torch.randn(1, 64, generator=g)}
    KW = dict(width=64, height=64, num_steps=4, seed=7, silent=True, output_type="latent")
    cond = torch.randn(1, 16, 64, generator=g)
    with pytest.raises(ValueError, match="controlnet_path"):
        make_pipe(None).generate(prompt, controlnet_cond=cond, **KW)
    pipe = make_pipe(net)
    with pytest.raises(ValueError, match="regions"):
        pipe.generate(prompt, controlnet_cond=cond, regions=[{"prompt": prompt, "box": (0, 0, 1, 1)}], **KW)
    with pytest.raises(ValueError, match="cache_threshold"):
        pipe.generate(prompt, controlnet_cond=cond, cache_threshold=0.1, **KW)
    with pytest.raises(ValueError, match="reference_image"):
        pipe.generate(prompt, controlnet_cond=cond, reference_image=torch.zeros(32, 32, 3, dtype=torch.uint8), **KW)
    with pytest.raises(ValueError, match="control_mode"):
        pipe.generate(prompt, controlnet_cond=cond, control_mode=1, **KW)
    with pytest.raises(ValueError, match="control_mode"):
        make_pipe(union).generate(prompt, controlnet_cond=cond, **KW)
    with pytest.raises(ValueError, match="control_guidance"):
        pipe.generate(prompt, controlnet_cond=cond, control_guidance_start=0.8, control_guidance_end=0.2, **KW)
    with pytest.raises(ValueError, match="controlnet_cond"):
        pipe.generate(prompt, controlnet_cond=cond[:, :5], **KW)
    with pytest.raises(RuntimeError, match="autoencoder"):
        pipe.generate(prompt, controlnet_image=torch.zeros(32, 32, 3, dtype=torch.uint8), **KW)
    pipe.model.calls.clear()
    # without controlnet_image the request is today's: no controlnet argument reaches the model
    pipe.generate(prompt, **KW)
    assert len(pipe.model.calls) == 1 and "controlnet" not in pipe.model.calls[0]
    pipe.model.calls.clear()
    pipe.generate(prompt, controlnet_cond=cond, controlnet_conditioning_scale=0.6, control_guidance_start=0.25, control_guidance_end=0.75, **KW)
    calls = pipe.model.calls
    assert [len(c["ts"]) - 1 for c in calls] == [1, 2, 1] and ["controlnet" in c for c in calls] == [False, True, False]
    assert calls[0]["ts"][-1] == calls[1]["ts"][0] and calls[1]["ts"][-1] == calls[2]["ts"][0]
    c = calls[1]["controlnet"]
    assert c.net is net and c.scale == 0.6 and c.mode is None and torch.equal(c.cond.float().cpu(), cond.to(torch.bfloat16).float())
    pipe.model.calls.clear()
    pipe.generate(prompt, controlnet_cond=cond, control_guidance_end=0.0, **KW)
    assert len(pipe.model.calls) == 1 and "controlnet" not in pipe.model.calls[0]


def test_api_fields():
    import api

    f = api.GenerateArgs.model_fields
    for k in ("controlnet_image", "controlnet_conditioning_scale", "control_mode", "control_guidance_start", "control_guidance_end"):
        assert k in f and f[k].default is None


def test_http_controlnet_fields():
    """the ControlNet fields reach generate() only when set; a request without them produces exactly today's keyword arguments"""
    import io

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
    r = c.post("/generate", json={**base, "controlnet_image": "edges.png", "controlnet_conditioning_scale": 0.7, "control_mode": 2,
                                  "control_guidance_start": 0.1, "control_guidance_end": 0.8})
    assert r.status_code == 200 and r.content.startswith(b"\xff\xd8")
    assert calls[-1]["controlnet_image"] == "edges.png" and calls[-1]["controlnet_conditioning_scale"] == 0.7 and calls[-1]["control_mode"] == 2
    assert calls[-1]["control_guidance_start"] == 0.1 and calls[-1]["control_guidance_end"] == 0.8 and "control_image" not in calls[-1]
    assert c.post("/generate", json={**base, "controlnet_image": "edges.png"}).status_code == 200
    assert "controlnet_conditioning_scale" not in calls[-1] and "control_mode" not in calls[-1]
    assert c.post("/generate", json={**base, "control_mode": -1}).status_code == 422
    assert c.post("/generate", json={**base, "control_guidance_end": 1.5}).status_code == 422
