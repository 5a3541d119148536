"""HTTP surface of the reference (api.py of aredden/flux-fp8-api) over the MI355X pipeline -- SURVEY.md §8(f) row 4.

Same two POST endpoints, request fields, defaults and status codes:
  /generate  GenerateArgs{prompt, width=720, height=1024, num_steps=24, guidance=3.5, seed=random in (0, MAX_RAND), strength=1.0,
             init_image=None (path or base64), reference_image=None (FLUX.1 Kontext edit; path or base64, passed on only when set),
             mask_image=None (FLUX.1 Fill: white = regenerate), control_image=None (FLUX.1 Depth / Canny: the depth or edge map),
             redux_image=None (FLUX.1 Redux image prompt) -- path or base64, each passed on only when set;
             ip_adapter_image=None (FLUX IP-Adapter image prompt: a path / base64 string or a list), ip_adapter_image_embeds=None ([n][768]),
             ip_adapter_scale=None (a float or one per double block), negative_ip_adapter_image=None, negative_ip_adapter_scale=None -- each
             passed on only when set;
             negative_prompt=None, true_cfg_scale=None, true_cfg_interval=None ([lo, hi]) -- true classifier-free guidance
             (FluxPipeline.generate), each passed on only when set;
             cache_threshold=None, cache_max_hits=None -- first-block step caching (FluxPipeline.generate), each passed on only when set;
             regions=None ([{prompt, box=[x0, y0, x1, y1] | mask}], regional prompts), regional_tokens=None -- each passed on only when
             set;
             inpaint_mask=None (path or base64; white = regenerate: masked-latent inpainting of init_image on any model),
             inpaint_differential=None (differential diffusion: the mask is a grey change map) -- each passed on only when set;
             sampler=None ("euler" | "heun" | "midpoint" | "ab2" | "dpmpp_2m"), sigma_schedule=None ("karras" | "exponential"),
             sigmas=None (the request's own descending list in (0, 1]; num_steps follows it) -- each passed on only when set;
             sampler also "euler_ancestral" | "dpmpp_2m_sde" (stochastic), with eta=None (0..1), s_noise=None (>= 0), noise_seed=None (the
             key of the in-kernel noise; default the request's seed) -- each passed on only when set;
             guidance_mode=None ("cfg" | "apg" | "cfg_zero_star"), guidance_rescale=None (0..1), apg_eta=None, apg_norm_threshold=None (>= 0),
             apg_momentum=None, zero_init_steps=None (>= 0) -- guidance shaping of true classifier-free guidance (FluxPipeline.generate; needs
             negative_prompt and true_cfg_scale > 1), each passed on only when set;
             source_prompt=None (FlowEdit: the prompt that describes init_image; `prompt` is then the target), source_guidance=None,
             edit_n_max=None (>= 0), edit_n_min=None (>= 0), edit_n_avg=None (>= 1) -- text-guided editing of init_image
             (FluxPipeline.generate), each passed on only when set;
             tile_size=None (an int or [height, width] in pixels), tile_overlap=None (>= 0, pixels), tile_weight=None ("cosine" | "uniform")
             -- tiled generation: a large canvas stepped from overlapping windows (FluxPipeline.generate), each passed on only when set;
             upscale=false, init_upscale=false -- the configured ESRGAN-family upscaler on the decoded pixels / on init_image
             (FluxPipeline.generate; needs config.upscaler_path), each passed on only when true;
             control_preprocess=None ("canny" | "gray" | "blur" | "depth_anything"), canny_low=None (>= 0), canny_high=None (>= 0),
             canny_l2=None, blur_sigma=None (> 0), depth_resolution=None (14..1036), depth_normalize=None ("minmax" | "raw") --
             control_image / controlnet_image is a PHOTO and the control map is made from it on the device
             (FluxPipeline.preprocess_control: a native Canny whose parity with OpenCV's is unpinned, PIL's luma, a Gaussian blur, the
             depth map of the Depth Anything estimator of config.depth_path), each passed on only when set;
             jpeg_encoder=None ("pil" | "native") -- who writes the response's JPEG: Pillow on the host, or the native encoder on the device
             (FluxPipeline.generate); passed on only when set, and unset means the config JSON's "jpeg_encoder" ("pil" unless given there);
             stream=None, preview_every=None (>= 0) -- progress, live previews and cancellation, see below;
             a region with both or neither of box / mask, or a box outside 0 <= x0 < x1 <= 1, is a 422}
             ->  image/jpeg stream of FluxPipeline.generate(**args)                                               (reference api.py:54-86)
             With stream=true the response is application/x-ndjson instead, one JSON object per line: for every model evaluation
               {"event": "progress", "evaluation", "num_evaluations", "step", "preview": <base64 JPEG at latent resolution, or null>}
             (a preview at every preview_every-th evaluation; none with preview_every unset or 0), then ONE final line
               {"event": "result", "image": <base64 JPEG>}  |  {"event": "cancelled"}  |  {"event": "error", "message"}.
             The request runs in a worker thread that feeds a queue; closing the response -- a client that disconnected -- sets a flag
             that the next on_step turns into a cancel, so an abandoned request frees its GPU within two model evaluations.
             preview_every without stream is a 422.
  /lora      LoraArgs{scale=1.0, path, name, action="load"|"unload"}  ->  {"status": "success"} | 400 invalid action | 500 with the
             exception text; unload uses `name` when given, else `path`                                         (reference api.py:89-122)
The app holds one pipeline in `app.state.model`; FastAPI runs these sync handlers on its threadpool, and the pipeline serialises
engine access with its own lock (modules/flux_model.py), so concurrent requests queue instead of interleaving.
"""
from __future__ import annotations

import base64
import io
import json
import queue
import random
import threading
from typing import List, Literal, Optional, Tuple, Union

from fastapi import FastAPI
from fastapi.responses import JSONResponse, StreamingResponse
from pydantic import BaseModel, Field

MAX_RAND = 2**32 - 1


class LoraArgs(BaseModel):
    scale: Optional[float] = 1.0
    path: Optional[str] = None
    name: Optional[str] = None
    action: Optional[Literal["load", "unload"]] = "load"


class LoraLoadResponse(BaseModel):
    status: Literal["success", "error"]
    message: Optional[str] = None


class RegionArgs(BaseModel):
    """one regional prompt: `prompt` holds inside `box` (x0, y0, x1, y1 in 0..1 of the image) or inside the white part of `mask` (path or base64)"""
    prompt: str
    box: Optional[Tuple[float, float, float, float]] = None
    mask: Optional[str] = None


class GenerateArgs(BaseModel):
    prompt: str
    width: Optional[int] = Field(default=720)
    height: Optional[int] = Field(default=1024)
    num_steps: Optional[int] = Field(default=24)
    guidance: Optional[float] = Field(default=3.5)
    seed: Optional[int] = Field(default_factory=lambda: random.randint(1, MAX_RAND - 1), gt=0, lt=MAX_RAND)
    strength: Optional[float] = 1.0
    init_image: Optional[str] = None
    reference_image: Optional[str] = None  # FLUX.1 Kontext instruction editing: the image to edit (path or base64, like init_image)
    mask_image: Optional[str] = None  # FLUX.1 Fill inpainting / outpainting: the mask of init_image to regenerate (white), path or base64
    control_image: Optional[str] = None  # FLUX.1 Depth / Canny: the depth map or edge map to follow, path or base64
    redux_image: Optional[str] = None  # FLUX.1 Redux: an image prompt (needs config redux_path / siglip_path), path or base64
    negative_prompt: Optional[str] = None  # true classifier-free guidance: what to steer away from ("" is valid); needs true_cfg_scale > 1
    true_cfg_scale: Optional[float] = None  # its scale (diffusers' name); guidance runs iff negative_prompt is set and this is > 1
    true_cfg_interval: Optional[Tuple[float, float]] = None  # [lo, hi], fractions of the steps that are guided (default: all)
    cache_threshold: Optional[float] = None  # first-block step caching: relative-L1 threshold of the first block's residual (off unless > 0)
    cache_max_hits: Optional[int] = None  # ... and the most cached steps in a row (0 = no bound)
    regions: Optional[List[RegionArgs]] = Field(default=None, min_length=1)  # regional prompts (FluxPipeline.generate)
    regional_tokens: Optional[int] = Field(default=None, gt=0, multiple_of=16)  # T5 rows kept per region prompt (default 128)
    inpaint_mask: Optional[str] = None  # masked-latent inpainting of init_image on any model: white = regenerate, path or base64
    inpaint_differential: Optional[bool] = None  # differential diffusion: inpaint_mask is a grey change map (lighter = changed more)
    controlnet_image: Optional[str] = None  # FLUX ControlNet (config controlnet_path): the edge map / depth map / pose to follow, path or base64
    controlnet_conditioning_scale: Optional[float] = None  # ... the strength of its residuals (default 1.0)
    ip_adapter_image: Optional[Union[str, List[str]]] = None  # FLUX IP-Adapter (config ip_adapter_path / clip_vision_path): image prompt(s), path or base64
    ip_adapter_image_embeds: Optional[List[List[float]]] = None  # ... or the CLIP image_embeds [n][768] already computed
    ip_adapter_scale: Optional[Union[float, List[float]]] = None  # ... its strength: a float, or one float per double block (default 1.0)
    negative_ip_adapter_image: Optional[Union[str, List[str]]] = None  # ... the negative branch's image(s) (default: black), with a negative prompt
    negative_ip_adapter_scale: Optional[Union[float, List[float]]] = None  # ... and its strength
    control_mode: Optional[int] = Field(default=None, ge=0)  # ... the control mode of a Union net
    control_guidance_start: Optional[float] = Field(default=None, ge=0.0, le=1.0)  # ... the fraction of the steps at which it switches on
    control_guidance_end: Optional[float] = Field(default=None, ge=0.0, le=1.0)  # ... and off (diffusers' names)
    sampler: Optional[Literal["euler", "heun", "midpoint", "ab2", "dpmpp_2m", "euler_ancestral", "dpmpp_2m_sde"]] = None  # the solver (default euler; fluxmi.solvers)
    sigma_schedule: Optional[Literal["karras", "exponential"]] = None  # re-space the schedule between its first and last non-zero sigma
    sigmas: Optional[List[float]] = Field(default=None, min_length=1)  # the request's own sigma list (diffusers' argument)
    eta: Optional[float] = Field(default=None, ge=0.0, le=1.0)  # stochastic samplers: the share of each step's noise that is re-drawn
    s_noise: Optional[float] = Field(default=None, ge=0.0)  # ... a factor on the drawn noise
    noise_seed: Optional[int] = Field(default=None, ge=0, lt=2 ** 64)  # ... the key of the in-kernel noise (default: the request's seed)
    guidance_mode: Optional[Literal["cfg", "apg", "cfg_zero_star"]] = None  # true CFG's combination rule (default cfg; FluxPipeline.generate)
    guidance_rescale: Optional[float] = Field(default=None, ge=0.0, le=1.0)  # ... CFG rescale (diffusers' name): 0 = off
    apg_eta: Optional[float] = None  # ... APG: the weight of the part of the guidance parallel to the prompt prediction (default 1)
    apg_norm_threshold: Optional[float] = Field(default=None, ge=0.0)  # ... APG: clip the guidance difference to this norm (0 = off)
    apg_momentum: Optional[float] = None  # ... APG: the running difference's momentum (0 = off)
    zero_init_steps: Optional[int] = Field(default=None, ge=0)  # ... CFG-Zero*'s zero-init: the first k model evaluations predict 0
    source_prompt: Optional[str] = None  # FlowEdit: the prompt that describes init_image; `prompt` is then the target prompt (FluxPipeline.generate)
    source_guidance: Optional[float] = None  # ... the distilled guidance of the source branch (default: guidance, which the target branch takes)
    edit_n_max: Optional[int] = Field(default=None, ge=0)  # ... the last edit_n_max steps are edited (default: every step)
    edit_n_min: Optional[int] = Field(default=None, ge=0)  # ... the last edit_n_min of them as a plain Euler tail on the target prompt (default 0)
    edit_n_avg: Optional[int] = Field(default=None, ge=1)  # ... model evaluations averaged per step (default 1)
    tile_size: Optional[Union[int, Tuple[int, int]]] = None  # tiled generation: the window in pixels, an int (square) or [height, width] (FluxPipeline.generate)
    tile_overlap: Optional[int] = Field(default=None, ge=0)  # ... the overlap of neighbouring windows in pixels (default: a quarter of the tile)
    tile_weight: Optional[str] = None  # ... "cosine" (default) | "uniform": how overlapping windows are blended
    upscale: Optional[bool] = False  # run the decoded pixels through the configured ESRGAN-family upscaler (config.upscaler_path): scale x the size
    init_upscale: Optional[bool] = False  # run init_image through it before the resize to width x height (the upscale + img2img workflow)
    control_preprocess: Optional[Literal["canny", "gray", "blur", "depth_anything"]] = None  # control_image / controlnet_image is a photo: make the map from it (FluxPipeline.preprocess_control)
    canny_low: Optional[int] = Field(default=None, ge=0)  # ... Canny's thresholds (defaults 100 / 200, diffusers' example values; BFL uses 50 / 200)
    canny_high: Optional[int] = Field(default=None, ge=0)
    canny_l2: Optional[bool] = None  # ... squared-gradient magnitudes instead of |dx| + |dy|
    blur_sigma: Optional[float] = Field(default=None, gt=0.0)  # ... the Gaussian's standard deviation in pixels (default 8; radius ceil(3 sigma) <= 64)
    depth_resolution: Optional[int] = Field(default=None, ge=14, le=1036)  # ... "depth_anything": the side the estimator sees (default 518)
    depth_normalize: Optional[Literal["minmax", "raw"]] = None  # ... its depth -> 0..255: each image's min..max (default) or clamp(depth, 0, 255)
    # who writes the response's JPEG: "pil" (Pillow on the host) or "native" (the device encoder, fluxmi.ops.jpeg_encode: the pixels never
    # leave the device uncompressed); unset = the configuration's jpeg_encoder ("pil" unless set there).  Previews stay on Pillow
    jpeg_encoder: Optional[Literal["pil", "native"]] = None
    stream: Optional[bool] = None  # answer with application/x-ndjson progress lines and a final result line instead of the JPEG
    preview_every: Optional[int] = Field(default=None, ge=0)  # ... with a latent-resolution preview at every k-th model evaluation (0 = none)


app = FastAPI(title="fluxmi")


def _preview_jpeg(preview) -> str:
    """uint8 [num_images, h, w, 3] -> base64 JPEG, the images stacked vertically like FluxPipeline.into_bytes"""
    import numpy as np
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(np.vstack(list(preview))).save(buf, format="JPEG", quality=90)
    return base64.b64encode(buf.getvalue()).decode("ascii")


def stream_events(model, kwargs):
    """The NDJSON lines of one streamed request (a generator of bytes).  `model.generate(**kwargs, on_step=...)` runs in a worker thread
    and feeds a queue; closing this generator -- what the server does when the client went away -- sets the flag that the next on_step
    turns into a cancel (it returns False), and the worker's remaining lines are dropped."""
    lines: "queue.Queue" = queue.Queue()
    gone = threading.Event()

    def on_step(info):
        if gone.is_set():
            return False
        pv = info.get("preview")
        lines.put({"event": "progress", "evaluation": int(info["evaluation"]), "num_evaluations": int(info["num_evaluations"]),
                   "step": int(info["step"]), "preview": None if pv is None else _preview_jpeg(pv)})
        return True

    def work():
        try:
            result = model.generate(**kwargs, on_step=on_step)
            data = result.getvalue() if hasattr(result, "getvalue") else bytes(result)
            lines.put({"event": "result", "image": base64.b64encode(data).decode("ascii")})
        except Exception as e:
            from fluxmi import GenerationCancelled

            lines.put({"event": "cancelled"} if isinstance(e, GenerationCancelled) else {"event": "error", "message": str(e)})
        finally:
            lines.put(None)

    worker = threading.Thread(target=work, name="fluxmi-stream", daemon=True)
    worker.start()
    try:
        while True:
            line = lines.get()
            if line is None:
                return
            yield (json.dumps(line) + "\n").encode("utf-8")
    finally:
        gone.set()


@app.post("/generate")
def generate(args: GenerateArgs):
    """JPEG bytes of one image; `init_image` + `strength` select img2img (flux_pipeline.py:399-420,459-523 of the reference);
    `reference_image` selects a FLUX.1 Kontext edit of that image, `mask_image` a FLUX.1 Fill inpainting of `init_image`, `control_image` a
    FLUX.1 Depth / Canny generation, `redux_image` a FLUX.1 Redux image prompt; `negative_prompt` + `true_cfg_scale` (+ `true_cfg_interval`)
    select true classifier-free guidance, `cache_threshold` (+ `cache_max_hits`) first-block step caching, `controlnet_image` (+ `controlnet_conditioning_scale`,
    `control_mode`, `control_guidance_start` / `_end`) a FLUX ControlNet, `ip_adapter_image` / `ip_adapter_image_embeds` (+ `ip_adapter_scale`,
    `negative_ip_adapter_image`, `negative_ip_adapter_scale`) a FLUX IP-Adapter, `guidance_mode` / `guidance_rescale` / `apg_*` /
    `zero_init_steps` guidance shaping of a guided request, `source_prompt` (+ `source_guidance`, `edit_n_max` / `_min` / `_avg`) a FlowEdit edit of
    `init_image` towards `prompt`, `tile_size` (+ `tile_overlap`, `tile_weight`) tiled generation of a large canvas, `upscale` / `init_upscale` the
    configured super-resolution network on the output / on `init_image`, `control_preprocess` (+ `canny_low` / `canny_high` / `canny_l2`,
    `blur_sigma`, `depth_resolution` / `depth_normalize`) the control map made on the device from a photo given as `control_image` /
    `controlnet_image` (a native Canny edge detector: exact integer arithmetic, parity with OpenCV's binary unpinned; PIL's luma; a Gaussian
    blur; a Depth Anything depth map, parity with BFL's post-processing unpinned).  Without them the call is exactly the reference's."""
    kwargs = args.model_dump()
    stream = bool(kwargs.pop("stream", None))
    if kwargs.get("preview_every") is None:
        kwargs.pop("preview_every", None)
    elif not stream:
        return JSONResponse(status_code=422, content={"status": "error", "message": "preview_every needs stream=true"})
    for k in ("reference_image", "mask_image", "control_image", "redux_image", "negative_prompt", "true_cfg_scale", "true_cfg_interval",
              "cache_threshold", "cache_max_hits", "regions", "regional_tokens", "inpaint_mask", "inpaint_differential", "controlnet_image",
              "controlnet_conditioning_scale", "control_mode", "control_guidance_start", "control_guidance_end", "sampler", "sigma_schedule",
              "sigmas", "eta", "s_noise", "noise_seed", "ip_adapter_image", "ip_adapter_image_embeds", "ip_adapter_scale",
              "negative_ip_adapter_image", "negative_ip_adapter_scale", "guidance_mode", "guidance_rescale", "apg_eta", "apg_norm_threshold",
              "apg_momentum", "zero_init_steps", "source_prompt", "source_guidance", "edit_n_max", "edit_n_min", "edit_n_avg", "tile_size",
              "tile_overlap", "tile_weight", "control_preprocess", "canny_low", "canny_high", "canny_l2", "blur_sigma", "depth_resolution",
              "depth_normalize", "jpeg_encoder"):
        if kwargs.get(k) is None:
            kwargs.pop(k, None)
    for k in ("upscale", "init_upscale"):  # passed on only when asked for
        if not kwargs.get(k):
            kwargs.pop(k, None)
    if "ip_adapter_image_embeds" in kwargs:
        import torch

        kwargs["ip_adapter_image_embeds"] = torch.tensor(kwargs["ip_adapter_image_embeds"], dtype=torch.float32)
    if "regions" in kwargs:
        regs = []
        for r in kwargs["regions"]:
            if (r.get("box") is None) == (r.get("mask") is None):
                return JSONResponse(status_code=422, content={"status": "error", "message": "a region takes exactly one of box and mask"})
            if r.get("box") is not None:
                x0, y0, x1, y1 = r["box"]
                if not (0.0 <= x0 < x1 <= 1.0 and 0.0 <= y0 < y1 <= 1.0):
                    return JSONResponse(status_code=422, content={"status": "error", "message": "a region box needs 0 <= x0 < x1 <= 1 and 0 <= y0 < y1 <= 1"})
                regs.append({"prompt": r["prompt"], "box": tuple(r["box"])})
            else:
                regs.append({"prompt": r["prompt"], "mask": r["mask"]})
        kwargs["regions"] = regs
    if stream:
        return StreamingResponse(stream_events(app.state.model, kwargs), media_type="application/x-ndjson")
    result = app.state.model.generate(**kwargs)
    return StreamingResponse(result, media_type="image/jpeg")


@app.post("/lora", response_model=LoraLoadResponse)
def lora_action(args: LoraArgs):
    """Fuse (`load`) or subtract-and-requantise (`unload`) a LoRA into the fp8 flow weights."""
    try:
        if args.action == "load":
            app.state.model.load_lora(args.path, args.scale, args.name)
        elif args.action == "unload":
            app.state.model.unload_lora(args.name if args.name else args.path)
        else:
            return JSONResponse(status_code=400, content={"status": "error", "message": f"Invalid action, expected 'load' or 'unload', got {args.action}"})
    except Exception as e:  # the reference reports every failure as a 500 with the message
        return JSONResponse(status_code=500, content={"status": "error", "message": str(e)})
    return JSONResponse(status_code=200, content={"status": "success"})
