"""FluxPipeline on MI355X -- the pipeline surface of the reference (flux_pipeline.py of aredden/flux-fp8-api)
over the native fluxmi denoise engine.

Hot path kept here: seed -> noise -> 2x2 patch packing + position ids ->
shifted schedule -> the Euler denoise loop (natively, hipGraph-replayed) -> unpack.
Same public names / kwargs / defaults as the reference: FluxPipeline.load_pipeline_from_config_path /
load_pipeline_from_config / generate / load_lora / unload_lora / compile / set_seed / get_schedule /
get_noise / prepare / unpack / vae_decode / into_bytes / load_init_image_if_needed / resize_center_crop / preprocess_latent.

SURVEY.md §8f rows 1-2 are built around it: the native VAE decoder (latents -> JPEG) and encoder (img2img: `init_image`, `strength`),
and the text conditioning (flux_emphasis.py prompt weighting over the native T5 / CLIP encoders of modules/conditioner.py) when
`config.text_enc_path` / `clip_path` point at local HF-layout directories.  Without them `generate()` takes the conditioning as
pre-computed embeddings (`prompt={"txt": [B,Lt,4096], "vec": [B,768]}`); it returns latents when no autoencoder is attached.
FLUX.1 Redux image prompts (`redux_image`) run through the native SigLIP + projector of modules/image_embedders.py when
`config.redux_path` / `siglip_path` point at local files.  CPU-offload flags are accepted
and ignored (meaningless with 288 GB of HBM).  `compile()` keeps the reference's warm-up/calibration protocol
(flux_pipeline.py:197-212) but never calls torch.compile: the fused kernels + hipGraph replace it.
"""
from __future__ import annotations

import io
import math
import random
from typing import Callable, List, Optional, Union

import numpy as np
import torch

import lora_loading  # noqa: F401  (same import side as the reference)
from fluxmi import dist as fdist
from fluxmi import ops, solvers
from modules.autoencoder import check_attention_mode
from util import (ModelSpec, ModelVersion, engine_flow_dtype, into_device, into_dtype, load_config_from_path, load_controlnet, load_depth_model, load_ip_adapter, load_upscaler,
                  load_models_from_config)

MAX_RAND = 2**32 - 1
CONTROL_PREPROCESSORS = ("canny", "gray", "blur", "depth_anything")  # generate(control_preprocess=...) / preprocess_control: the maps made from a photo
JPEG_ENCODERS = ("pil", "native")  # generate(jpeg_encoder=...) / ModelSpec.jpeg_encoder: Pillow on the host, or fluxmi.ops.jpeg_encode on the device
GUIDANCE_MODES = ("cfg", "apg", "cfg_zero_star")  # generate(guidance_mode=...): the rule that combines the two branches of true CFG

# FLUX.1 Kontext's preferred reference resolutions, (width, height) (BFL flux, src/flux/sampling.py)
KONTEXT_PREFERRED_RESOLUTIONS = [
    (672, 1568), (688, 1504), (720, 1456), (752, 1392), (800, 1328), (832, 1248), (880, 1184), (944, 1104), (1024, 1024),
    (1104, 944), (1184, 880), (1248, 832), (1328, 800), (1392, 752), (1456, 720), (1504, 688), (1568, 672),
]


def kontext_reference_size(width: int, height: int):
    """-> (w, h, w_l, h_l): the preferred Kontext resolution closest in aspect ratio to a `width` x `height` image, and its latent size
    (w_l = 2 * int(w / 16), h_l = 2 * int(h / 16)).  Ties go to the smaller (width, height) pair, as min() over tuples does."""
    a = width / height
    _, w, h = min((abs(a - w / h), w, h) for (w, h) in KONTEXT_PREFERRED_RESOLUTIONS)
    return w, h, 2 * int(w / 16), 2 * int(h / 16)


def kontext_reference_ids(bs: int, h_l: int, w_l: int, device=None, dtype=torch.bfloat16) -> torch.Tensor:
    """Position ids of the reference tokens, [bs, (h_l/2) * (w_l/2), 3]: make_img_ids over the (h_l/2) x (w_l/2) grid (axis 1 the row, axis 2
    the column) with axis 0 set to 1, which tells the model these tokens are the reference, not the image being generated."""
    ids = FluxPipeline.make_img_ids(bs, h_l // 2, w_l // 2, device, dtype)
    ids[..., 0] = 1
    return ids


# ---- regional prompts: token-group attention masks (include/fluxmi.h, fluxmi_attention_grouped) --------------------------------------
ATTN_GROUPS = 16  # key groups of a descriptor table


def region_token_grid(region: dict, height: int, width: int) -> torch.Tensor:
    """One entry of generate(regions=...) -> bool [height/16, width/16]: which image tokens the region covers.  `box` = (x0, y0, x1, y1)
    in 0..1 of the image, or `mask` = an image / array / tensor (white = inside; any size, resized by area averaging).  Both are
    area-averaged to the token grid and thresholded at 0.5.  A region that covers no token is refused."""
    h, w = height // 16, width // 16
    if not isinstance(region, dict) or ("box" in region) == ("mask" in region):
        raise ValueError("fluxmi: a region needs a 'prompt' and exactly one of 'box' (x0, y0, x1, y1 in 0..1) and 'mask'")
    if "box" in region:
        try:
            x0, y0, x1, y1 = (float(v) for v in region["box"])
        except (TypeError, ValueError):
            raise ValueError(f"fluxmi: region box {region['box']!r}: expected (x0, y0, x1, y1)") from None
        if not (0.0 <= x0 < x1 <= 1.0 and 0.0 <= y0 < y1 <= 1.0):
            raise ValueError(f"fluxmi: region box {region['box']!r}: expected 0 <= x0 < x1 <= 1 and 0 <= y0 < y1 <= 1")
        # covered fraction of every token cell = (overlap of [x0 w, x1 w] with [j, j + 1]) x (the same in y)
        cov = lambda a, b, n: (torch.minimum(torch.arange(1, n + 1, dtype=torch.float64), torch.tensor(b * n, dtype=torch.float64))
                               - torch.maximum(torch.arange(0, n, dtype=torch.float64), torch.tensor(a * n, dtype=torch.float64))).clamp_(min=0)
        frac = cov(y0, y1, h)[:, None] * cov(x0, x1, w)[None, :]
    else:
        m = region["mask"]
        if hasattr(m, "convert"):  # PIL
            m = np.array(m.convert("L"))
        m = torch.as_tensor(np.asarray(m) if not isinstance(m, torch.Tensor) else m)
        # 8-bit images are 0..255; bool masks and the 0 / 1 bytes of a bilevel ('1') image are 0..1 already, like float masks
        scale = 255.0 if m.dtype == torch.uint8 and m.numel() and int(m.max()) > 1 else 1.0
        m = m.to(torch.float64) / scale
        if m.dim() == 3:
            m = m.mean(-1) if m.shape[-1] in (1, 3, 4) else m.mean(0)
        if m.dim() != 2 or m.numel() == 0:
            raise ValueError(f"fluxmi: region mask of shape {tuple(m.shape)}: expected [H, W] (or an image)")
        frac = torch.nn.functional.adaptive_avg_pool2d(m[None, None], (h, w))[0, 0]
    grid = frac >= 0.5
    if not bool(grid.any()):
        raise ValueError("fluxmi: a region covers no image token (16 x 16 pixels each) at this size")
    return grid


def build_region_groups(n_base: int, regional_tokens: int, region_grids: torch.Tensor, n_ref: int = 0, negative: bool = False) -> torch.Tensor:
    """The descriptor table of ONE sample of a regional request, int32 [L] (include/fluxmi.h: g | P << 16; query i attends key j iff bit
    g_j of P_i), for the joint sequence
        [ base text (n_base rows: T5 + Redux tokens) | region 1 text | .. | region R text (regional_tokens rows each) | image tokens
          (h w, row-major) | n_ref Kontext reference rows ].
    region_grids: bool [R, h, w], which image tokens each region covers (region_token_grid).
    Key groups: 0 = base text; r = 1..R the text of region r; then one group per distinct COVERAGE PATTERN of the image tokens (the set
    of regions that cover a token), in ascending order of the pattern read as a bit set -- uncovered tokens and reference rows have the
    pattern "none".  More than 16 groups are refused.
    Permissions: a base-text query sees group 0 and every image group; a text query of region r sees group r and the image groups whose
    pattern contains r; an image query of pattern S sees group 0, the text groups of S and EVERY image group (image-to-image attention
    stays dense).  negative=True (the negative branch of true classifier-free guidance): every query loses the region text groups and a
    region's text rows see only themselves, so their content is inert.  Every query admits its own group."""
    grids = torch.as_tensor(region_grids).bool()
    if grids.dim() != 3 or grids.shape[0] < 1:
        raise ValueError(f"fluxmi: region grids of shape {tuple(grids.shape)}: expected [R >= 1, h, w]")
    R = grids.shape[0]
    if n_base < 0 or n_ref < 0 or regional_tokens < 1:
        raise ValueError("fluxmi: n_base, n_ref >= 0 and regional_tokens >= 1 expected")
    if R + 2 > ATTN_GROUPS:
        raise ValueError(f"fluxmi: {R} regions need {R + 2} or more attention groups; at most {ATTN_GROUPS} exist (base text + one per region "
                         "text + one per distinct overlap pattern)")
    for r in range(R):
        if not bool(grids[r].any()):
            raise ValueError(f"fluxmi: region {r} covers no image token")
    pattern = (grids.flatten(1).long() << torch.arange(R)[:, None]).sum(0)  # [h w] bit r = region r + 1 covers the token
    if n_ref:
        pattern = torch.cat((pattern, torch.zeros(n_ref, dtype=torch.long)))
    pats = torch.unique(pattern)  # ascending
    n_groups = 1 + R + pats.numel()
    if n_groups > ATTN_GROUPS:
        raise ValueError(f"fluxmi: the regions need {n_groups} attention groups (1 base text + {R} region texts + {pats.numel()} distinct "
                         f"overlap patterns of the image tokens); at most {ATTN_GROUPS} exist -- use fewer or less overlapping regions")
    img_group = 1 + R + torch.searchsorted(pats, pattern)
    img_bits = sum(1 << (1 + R + i) for i in range(pats.numel()))
    txt_of = lambda p: (int(p) << 1)  # pattern bit r -> text group r + 1
    group = torch.cat((torch.zeros(n_base, dtype=torch.long), torch.arange(1, R + 1).repeat_interleave(regional_tokens), img_group))
    if negative:
        perm_region = [1 << r for r in range(1, R + 1)]
        perm_img = torch.full_like(pattern, 1 | img_bits)
    else:
        perm_region = [(1 << r) | sum(1 << (1 + R + i) for i, p in enumerate(pats.tolist()) if (p >> (r - 1)) & 1) for r in range(1, R + 1)]
        perm_img = (pattern << 1) | 1 | img_bits
    perm = torch.cat((torch.full((n_base,), 1 | img_bits, dtype=torch.long),
                      torch.tensor(perm_region, dtype=torch.long).repeat_interleave(regional_tokens), perm_img))
    d = group | (perm << 16)
    assert bool(((perm >> group) & 1).all())
    return torch.where(d >= 1 << 31, d - (1 << 32), d).to(torch.int32)


class FluxPipeline:
    def __init__(self, name: str, offload: bool = False, clip=None, t5=None, model=None, ae=None,
                 dtype: torch.dtype = torch.float16, verbose: bool = False, flux_device="cuda:0", ae_device="cuda:1",
                 clip_device="cuda:1", t5_device="cuda:1", config: ModelSpec = None, debug: bool = False, redux=None,
                 controlnet=None, ip_adapter=None, upscaler=None, depth_model=None):
        if config is None:
            raise ValueError("ModelSpec config is required!")
        self.debug, self.name, self.verbose, self.offload = debug, name, verbose, offload
        self.device_flux = into_device(flux_device)
        self.device_ae, self.device_clip, self.device_t5 = into_device(ae_device), into_device(clip_device), into_device(t5_device)
        self.dtype = into_dtype(dtype)
        self.clip, self.t5, self.model, self.ae = clip, t5, model, ae
        self.vae_attention = check_attention_mode(getattr(config, "vae_attention", "gemm"))
        if ae is not None:
            ae.attention = self.vae_attention
        self.redux = redux  # FLUX.1 Redux image encoder (modules/image_embedders.ReduxImageEncoder) or None
        self.controlnet = controlnet  # FLUX ControlNet (modules/controlnet.FluxControlNet, config.controlnet_path) or None
        self.ip_adapter = ip_adapter  # FLUX IP-Adapter (modules/ip_adapter.IPAdapter, config.ip_adapter_path / clip_vision_path) or None
        self.upscaler = upscaler  # ESRGAN-family super-resolution network (modules/upscaler.RRDBNet, config.upscaler_path) or None
        self.depth_model = depth_model  # Depth Anything depth estimator (modules/depth.DepthAnythingNative, config.depth_path) or None
        self.rng = torch.Generator(device="cpu")
        self.ae_dtype = torch.bfloat16
        self.config = config
        self.offload_text_encoder = config.offload_text_encoder
        self.offload_vae = config.offload_vae
        self.offload_flow = config.offload_flow
        self.model.to(self.device_flux)
        if config.compile_blocks or config.compile_extras:
            self.compile()

    # ---- seeds / noise / schedule (reference flux_pipeline.py:126-149, 314-371) -------------------------------
    def set_seed(self, seed: int | None = None, seed_globally: bool = False):
        if isinstance(seed, (int, float)):
            seed = int(abs(seed)) % MAX_RAND
        elif isinstance(seed, str):
            try:
                seed = abs(int(seed)) % MAX_RAND
            except Exception:
                seed = abs(self.rng.seed()) % MAX_RAND
        else:
            seed = abs(self.rng.seed()) % MAX_RAND
        generator = torch.Generator(self.device_flux).manual_seed(seed)
        if seed_globally:
            torch.cuda.manual_seed_all(seed)
            np.random.seed(seed)
            random.seed(seed)
        return generator, seed

    def time_shift(self, mu: float, sigma: float, t: torch.Tensor):
        return math.exp(mu) / (math.exp(mu) + (1 / t - 1) ** sigma)

    def get_lin_function(self, x1: float = 256, y1: float = 0.5, x2: float = 4096, y2: float = 1.15) -> Callable[[float], float]:
        m = (y2 - y1) / (x2 - x1)
        b = y1 - m * x1
        return lambda x: m * x + b

    def get_schedule(self, num_steps: int, image_seq_len: int, base_shift: float = 0.5, max_shift: float = 1.15,
                     shift: bool = True) -> list[float]:
        timesteps = torch.linspace(1, 0, num_steps + 1)
        if shift:
            mu = self.get_lin_function(y1=base_shift, y2=max_shift)(image_seq_len)
            timesteps = self.time_shift(mu, 1.0, timesteps)
        return timesteps.tolist()

    def get_noise(self, num_samples: int, height: int, width: int, generator: torch.Generator, dtype=None, device=None) -> torch.Tensor:
        device = self.device_flux if device is None else device
        dtype = self.dtype if dtype is None else dtype
        return torch.randn(num_samples, 16, 2 * math.ceil(height / 16), 2 * math.ceil(width / 16), device=device, dtype=dtype,
                           generator=generator, requires_grad=False)

    # ---- img2img entry (reference flux_pipeline.py:399-420, 450-523) ---------------------------------------------------
    def load_init_image_if_needed(self, init_image):
        """str (path or base64 / data-URL) | PIL.Image | np.ndarray -> uint8 HWC tensor; a torch.Tensor is returned as is."""
        from base64 import standard_b64decode

        from PIL import Image

        if isinstance(init_image, str):
            try:
                init_image = Image.open(init_image)
            except Exception:
                init_image = Image.open(io.BytesIO(standard_b64decode(init_image.split(",")[-1])))
            init_image = torch.from_numpy(np.array(init_image)).type(torch.uint8)
        elif isinstance(init_image, np.ndarray):
            init_image = torch.from_numpy(init_image).type(torch.uint8)
        elif isinstance(init_image, Image.Image):
            init_image = torch.from_numpy(np.array(init_image)).type(torch.uint8)
        return init_image

    @staticmethod
    def resize_center_crop(img: torch.Tensor, height: int, width: int) -> torch.Tensor:
        """[..., C, H, W] -> shorter edge resized to min(width, height), then centre-cropped (zero-padded where still smaller) to
        (height, width).  The reference calls torchvision's TF.resize / TF.center_crop (flux_pipeline.py:450-457); torchvision is not in
        this image, so the same arithmetic is restated: antialiased bilinear in fp32 (torchvision upcasts bf16), long edge =
        int(size * long / short), crop origin = int(round((H - h) / 2))."""
        size = min(width, height)
        H, W = img.shape[-2:]
        short, long_ = (W, H) if W <= H else (H, W)
        if short != size:
            new_long = int(size * long_ / short)
            nh, nw = (new_long, size) if W <= H else (size, new_long)
            lead = img.shape[:-3]
            r = torch.nn.functional.interpolate(img.reshape(-1, *img.shape[-3:]).float(), size=(nh, nw), mode="bilinear", align_corners=False,
                                                antialias=True)
            img = r.to(img.dtype).reshape(*lead, *r.shape[-3:])
            H, W = nh, nw
        if width > W or height > H:
            pl, pt = (width - W) // 2 if width > W else 0, (height - H) // 2 if height > H else 0
            pr, pb = (width - W + 1) // 2 if width > W else 0, (height - H + 1) // 2 if height > H else 0
            img = torch.nn.functional.pad(img, (pl, pr, pt, pb))
            H, W = img.shape[-2:]
        top, left = int(round((H - height) / 2.0)), int(round((W - width) / 2.0))
        return img[..., top:top + height, left:left + width]

    @torch.inference_mode()
    def preprocess_latent(self, init_image=None, height: int = 720, width: int = 1024, num_steps: int = 20, strength: float = 1.0,
                          generator: torch.Generator = None, num_images: int = 1, noise: Optional[torch.Tensor] = None, sigmas=None,
                          sigma_schedule=None, image_seq_len: Optional[int] = None):
        """reference flux_pipeline.py:459-523: noise + schedule; with an init image: VAE-encode it, start the schedule at
        t_idx = int((1 - strength) * num_steps) and blend x = t * noise + (1 - t) * latent."""
        return self.preprocess_latent_parts(init_image, height, width, num_steps, strength, generator, num_images, noise, sigmas, sigma_schedule,
                                            image_seq_len)[:2]

    @torch.inference_mode()
    def preprocess_latent_parts(self, init_image=None, height: int = 720, width: int = 1024, num_steps: int = 20, strength: float = 1.0,
                                generator: torch.Generator = None, num_images: int = 1, noise: Optional[torch.Tensor] = None, sigmas=None,
                                sigma_schedule=None, image_seq_len: Optional[int] = None):
        """preprocess_latent, with what it blends: -> (x, timesteps, latent, noise).  `latent` = the VAE latent of `init_image` [num_images,
        16, H/8, W/8] in the flow dtype (None without an init image: one encode per request), `noise` = the pure draw before the blend.
        Masked-latent inpainting re-blends these two at every step (Flux.denoise).  `sigmas` (num_steps + 1 values ending at 0) replaces
        get_schedule's list; `sigma_schedule` ("karras" / "exponential") re-spaces either one (fluxmi.solvers.sigma_schedule).
        `image_seq_len`: the sequence length the schedule's shift follows (None: the latent's own; a tiled request passes its window's)."""
        if init_image is not None:
            if self.ae is None:
                raise RuntimeError("fluxmi: img2img needs an autoencoder (config.ae_path) -- none is attached")
            if isinstance(init_image, np.ndarray):
                init_image = torch.from_numpy(init_image)
            init_image = init_image.permute(2, 0, 1).contiguous().to(self.device_ae, dtype=self.ae_dtype).div(127.5).sub(1)[None, ...]
            init_image = self.resize_center_crop(init_image, height, width)
            init_image = self.ae.encode(init_image).to(dtype=self.dtype, device=self.device_flux).repeat(num_images, 1, 1, 1)
        x = self.get_noise(num_images, height, width, generator=generator) if noise is None else noise
        x = x.to(device=self.device_flux, dtype=self.dtype)
        timesteps = self.get_schedule(num_steps, x.shape[-1] * x.shape[-2] // 4 if image_seq_len is None else int(image_seq_len),
                                      shift=(self.name != "flux-schnell"))
        if sigmas is not None:
            if len(sigmas) != num_steps + 1:
                raise ValueError(f"fluxmi: {len(sigmas)} sigmas for {num_steps} steps (one more than steps)")
            timesteps = [float(v) for v in sigmas]
        if sigma_schedule is not None:
            timesteps = solvers.sigma_schedule(sigma_schedule, timesteps)
        if init_image is not None:
            t_idx = int((1 - strength) * num_steps)
            t = timesteps[t_idx]
            timesteps = timesteps[t_idx:]
            pure, x = x, t * x + (1.0 - t) * init_image
            return x, timesteps, init_image, pure
        return x, timesteps, None, x

    @torch.inference_mode()
    def prepare_inpaint_mask(self, inpaint_mask, height: int, width: int, differential: bool = False) -> torch.Tensor:
        """The mask of a masked-latent inpainting request -> bf16 [1, Li, 64] on the flow device, one value per element of the packed latent
        (1 = regenerate, 0 = keep; Flux.denoise's `inpaint_mask`):
          1. `inpaint_mask` in any form load_init_image_if_needed takes (path, base64 / data-URL, PIL image, uint8 array or tensor) is
             converted to single-channel "L" as PIL does, then float / 255: [1, 1, H, W].  White = regenerate, black = keep;
          2. brought to (height, width) with img2img's resize_center_crop when its size differs;
          3. the mean over each 8 x 8 pixel block gives one value per latent pixel: [1, 1, H/8, W/8];
          4. binarised at >= 0.5 (a latent pixel is regenerated when at least half of its block is white); with `differential` the means
             are kept as the grey change map of differential diffusion;
          5. repeated over the 16 latent channels and packed 2 x 2 like the latents."""
        if isinstance(inpaint_mask, torch.Tensor) and inpaint_mask.dtype != torch.uint8:
            raise TypeError(f"fluxmi: an inpaint_mask tensor must be uint8 (HW or HWC), got {inpaint_mask.dtype}")
        if not isinstance(inpaint_mask, (str, np.ndarray, torch.Tensor)) and not hasattr(inpaint_mask, "convert"):
            raise TypeError(f"fluxmi: inpaint_mask must be a path / base64 string, a PIL image or a uint8 array / tensor, got {type(inpaint_mask).__name__}")
        m = torch.from_numpy(np.array(self._rgb_uint8(inpaint_mask).convert("L"))).float().div(255.0)[None, None]
        if tuple(m.shape[-2:]) != (height, width):
            m = self.resize_center_crop(m, height, width)
        m = m.reshape(1, 1, height // 8, 8, width // 8, 8).mean(dim=(3, 5))
        if not differential:
            m = (m >= 0.5).float()
        return self.pack(m.repeat(1, 16, 1, 1)).to(device=self.device_flux, dtype=torch.bfloat16).contiguous()

    @staticmethod
    def inpaint_thresholds(n_steps: int) -> list:
        """Differential diffusion's schedule over the n steps a request really runs: step i regenerates what is lighter than
        thr_i = 1 - (i + 1) / n.  White (1) is free from the first step, black (0) is kept to the end (thr_{n-1} = 0, strict compare), a
        grey g is released for roughly the last fraction g of the steps."""
        return [1.0 - (i + 1) / n_steps for i in range(n_steps)]

    # ---- FLUX.1 Kontext reference image ------------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def prepare_kontext_reference(self, reference_image, num_images: int = 1, generator: torch.Generator = None):
        """The reference image of an instruction edit (FLUX.1 Kontext [dev]) -> (img_cond_seq [num_images, Lc, 64], img_cond_seq_ids
        [num_images, Lc, 3]) in the flow dtype on the flow device.  The semantics of BFL's prepare_kontext / denoise (src/flux/sampling.py),
        kept here in one place:
          1. preprocessing: a = W / H of the input image picks (w, h) = min((|a - w/h|, w, h)) over KONTEXT_PREFERRED_RESOLUTIONS; the
             latent size is w_l = 2 * int(w / 16), h_l = 2 * int(h / 16); the RGB image is resized to (8 w_l, 8 h_l) with PIL LANCZOS, scaled
             to [-1, 1], VAE-encoded (the native encoder img2img uses) and packed 2x2 like the noise: Lc = (h_l / 2) * (w_l / 2);
          2. position ids: make_img_ids over the (h_l / 2) x (w_l / 2) grid with axis 0 set to 1;
          3. forward: the reference tokens are appended to the image stream of every step; only the noisy tokens are predicted and stepped
             (img = img + (t_prev - t_curr) * pred[:, :Li]); the reference tokens never change;
          4. schedule: get_schedule(num_steps, Li) counts the noisy tokens only (generate() does);
          5. the output size is the requested width / height, independent of the reference's snapped size.
        The encoder's Gaussian sample is drawn from `generator` ([1, z_channels, h_l, w_l], one draw shared by the num_images copies);
        generate() passes the request's seeded generator AFTER the noise has been drawn from it, so one seed gives one result.
        `reference_image`: anything load_init_image_if_needed takes (path, base64 / data-URL, PIL image, HWC uint8 array or tensor)."""
        from PIL import Image

        if self.ae is None:
            raise RuntimeError("fluxmi: a Kontext reference image needs an autoencoder (config.ae_path) -- none is attached")
        ref = self.load_init_image_if_needed(reference_image)
        if isinstance(ref, torch.Tensor):
            ref = ref.detach().cpu()
            if ref.dtype != torch.uint8:
                raise TypeError(f"fluxmi: a reference image tensor must be uint8 HWC, got {ref.dtype}")
            ref = ref.numpy()
        pil = Image.fromarray(np.asarray(ref)).convert("RGB")
        width, height = pil.size
        _, _, w_l, h_l = kontext_reference_size(width, height)
        pil = pil.resize((8 * w_l, 8 * h_l), Image.LANCZOS)
        x = torch.from_numpy(np.array(pil)).permute(2, 0, 1).float().div(127.5).sub(1.0)[None]
        x = x.to(self.device_ae, dtype=self.ae_dtype)
        f = 1 << (self.ae.encoder.num_resolutions - 1)  # the encoder's downsampling (8 for every Flux autoencoder)
        z_ch = self.ae.encoder.conv_out.out_channels // 2
        gen_dev = generator.device if generator is not None else self.device_ae
        eps = torch.randn(1, z_ch, 8 * h_l // f, 8 * w_l // f, generator=generator, device=gen_dev, dtype=torch.float32)
        z = self.ae.encode(x, noise=eps.to(self.device_ae))
        cond = self.pack(z.to(device=self.device_flux, dtype=self.dtype)).repeat(num_images, 1, 1)
        ids = kontext_reference_ids(num_images, h_l, w_l, self.device_flux, self.dtype)
        return cond.contiguous(), ids

    # ---- FLUX.1 Fill / Depth / Canny channel conditioning ------------------------------------------------------------------------------
    def conditioning_kind(self) -> Optional[str]:
        """None (text-to-image: in_channels == out_channels), "fill" (FLUX.1 Fill [dev]: 320 conditioning channels) or "control" (FLUX.1
        Depth / Canny [dev]: 64).  Any other split is refused."""
        extra = getattr(self.model, "in_channels", 64) - getattr(self.model, "out_channels", getattr(self.model, "in_channels", 64))
        if extra == 0:
            return None
        kind = {320: "fill", 64: "control"}.get(extra)
        if kind is None:
            raise ValueError(f"fluxmi: a model with {extra} conditioning channels per token is neither FLUX.1 Fill (320) nor Depth / Canny (64)")
        return kind

    def _rgb_uint8(self, image) -> torch.Tensor:
        """any form load_init_image_if_needed takes -> PIL image (uint8 tensors only, like a Kontext reference)"""
        from PIL import Image

        im = self.load_init_image_if_needed(image)
        if isinstance(im, torch.Tensor):
            im = im.detach().cpu()
            if im.dtype != torch.uint8:
                raise TypeError(f"fluxmi: a conditioning image tensor must be uint8 HWC, got {im.dtype}")
            im = im.numpy()
        return im if isinstance(im, Image.Image) else Image.fromarray(np.asarray(im))

    def _encode_sampled(self, x: torch.Tensor, generator: torch.Generator = None) -> torch.Tensor:
        """VAE-encode x [1, 3, H, W] in [-1, 1] with the Gaussian sample [1, z_channels, H/8, W/8] drawn from `generator` -> bf16 latents"""
        f = 1 << (self.ae.encoder.num_resolutions - 1)  # the encoder's downsampling (8 for every Flux autoencoder)
        z_ch = self.ae.encoder.conv_out.out_channels // 2
        gen_dev = generator.device if generator is not None else self.device_ae
        eps = torch.randn(1, z_ch, x.shape[-2] // f, x.shape[-1] // f, generator=generator, device=gen_dev, dtype=torch.float32)
        return self.ae.encode(x.to(self.device_ae, dtype=self.ae_dtype), noise=eps.to(self.device_ae)).to(torch.bfloat16)

    @staticmethod
    def pack_fill_mask(mask: torch.Tensor) -> torch.Tensor:
        """mask [B, 1, H, W] in [0, 1] -> bf16 [B, (H/16) * (W/16), 256]: each 8 x 8 pixel block of a latent pixel becomes 64 channels (BFL:
        rearrange(mask[:, 0], "b (h ph) (w pw) -> b (ph pw) h w", ph=8, pw=8)), then packed 2 x 2 like the latents."""
        m = mask[:, 0].to(torch.bfloat16)
        b, H, W = m.shape
        m = m.reshape(b, H // 8, 8, W // 8, 8).permute(0, 2, 4, 1, 3).reshape(b, 64, H // 8, W // 8)
        return FluxPipeline.pack(m)

    @torch.inference_mode()
    def prepare_fill_conditioning(self, image, mask, height: int, width: int, num_images: int = 1,
                                  generator: torch.Generator = None) -> torch.Tensor:
        """FLUX.1 Fill [dev] (inpainting / outpainting) -> img_cond bf16 [num_images, Li, 320] on the flow device.  The semantics of BFL's
        prepare_fill / denoise (src/flux/sampling.py), kept here in one place:
          1. the RGB image goes to float / 127.5 - 1, [1, 3, H, W]; the mask is converted to single-channel "L" as PIL does, then
             float / 255, [1, 1, H, W].  White (1) means "regenerate", black (0) "keep";
          2. masked = image * (1 - mask), VAE-encoded with its Gaussian sample, cast to bf16 and packed 2 x 2: [1, Li, 64];
          3. bf16(mask[:, 0]) is rearranged "b (h ph) (w pw) -> b (ph pw) h w" (ph = pw = 8) and packed 2 x 2: [1, Li, 256]
             (pack_fill_mask);
          4. img_cond = cat(latents, mask, -1), [1, Li, 320], repeated over the batch; it is appended to the channels of every token of every
             step, the model predicts the 64 noisy channels and only they are stepped.
        Ours, not BFL's: image and mask are brought to (width, height) with img2img's resize_center_crop (skipped when the size already
        matches, so a correctly sized input passes unchanged).  The encoder's sample is drawn from `generator` ([1, 16, H/8, W/8], one draw
        shared by the copies); generate() passes the request's generator AFTER the noise, so one seed gives one image.  Outpainting is the same
        call on an image padded to the new size, with a mask that is white over the padding.  BFL recommends guidance 30 and about 50 steps.
        `image` / `mask`: anything load_init_image_if_needed takes (path, base64 / data-URL, PIL image, uint8 array or tensor)."""
        if self.ae is None:
            raise RuntimeError("fluxmi: FLUX.1 Fill conditioning needs an autoencoder (config.ae_path) -- none is attached")
        img = torch.from_numpy(np.array(self._rgb_uint8(image).convert("RGB"))).float().div(127.5).sub(1.0).permute(2, 0, 1)[None]
        m = torch.from_numpy(np.array(self._rgb_uint8(mask).convert("L"))).float().div(255.0)[None, None]
        if tuple(img.shape[-2:]) != (height, width):
            img = self.resize_center_crop(img, height, width)
        if tuple(m.shape[-2:]) != (height, width):
            m = self.resize_center_crop(m, height, width)
        z = self._encode_sampled(img * (1.0 - m), generator)
        cond = torch.cat((self.pack(z), self.pack_fill_mask(m).to(z.device)), -1)
        return cond.to(self.device_flux).repeat(num_images, 1, 1).contiguous()

    @torch.inference_mode()
    def prepare_control_conditioning(self, control_image, height: int, width: int, num_images: int = 1,
                                     generator: torch.Generator = None) -> torch.Tensor:
        """FLUX.1 Depth / Canny [dev] -> img_cond bf16 [num_images, Li, 64] on the flow device (BFL's prepare_control, src/flux/sampling.py):
        the RGB control image is resized to (width, height) with PIL LANCZOS, goes to float / 127.5 - 1, is VAE-encoded with its Gaussian
        sample (drawn from `generator` after the noise, as in prepare_fill_conditioning), cast to bf16 and packed 2 x 2.  `control_image` is
        the depth map or edge map itself.  Either can be made from a photo by preprocess_control (generate's `control_preprocess`):
        "canny", a native Canny where BFL calls OpenCV's, and "depth_anything", the native Depth Anything estimator of config.depth_path."""
        from PIL import Image

        if self.ae is None:
            raise RuntimeError("fluxmi: FLUX.1 Depth / Canny conditioning needs an autoencoder (config.ae_path) -- none is attached")
        pil = self._rgb_uint8(control_image).convert("RGB").resize((width, height), Image.LANCZOS)
        x = torch.from_numpy(np.array(pil)).float().div(127.5).sub(1.0).permute(2, 0, 1)[None]
        cond = self.pack(self._encode_sampled(x, generator))
        return cond.to(self.device_flux).repeat(num_images, 1, 1).contiguous()

    @torch.inference_mode()
    def prepare_controlnet_conditioning(self, controlnet_image, height: int, width: int, num_images: int = 1,
                                        generator: torch.Generator = None) -> torch.Tensor:
        """A ControlNet's `cond` bf16 [num_images, Li, 64] on the flow device (diffusers' FluxControlNetPipeline.prepare_image + the latent
        handling of its __call__): the control image, in any form `init_image` takes, is resized like `control_image`, VAE-encoded (its
        Gaussian sample drawn from `generator` after the noise), shifted and scaled, cast to bf16 and packed 2 x 2.  `controlnet_image` is
        the edge map / depth map / pose itself.  Canny edges, gray, blur and a Depth Anything depth map (config.depth_path) can be made from
        a photo by preprocess_control (generate's `control_preprocess`); a pose preprocessor is not part of this project."""
        if self.ae is None:
            raise RuntimeError("fluxmi: controlnet_image needs an autoencoder (config.ae_path) -- none is attached; pass controlnet_cond")
        return self.prepare_control_conditioning(controlnet_image, height, width, num_images=num_images, generator=generator)

    # ---- control-map preprocessors (csrc/preprocess.hip) ---------------------------------------------------------------------------------
    def _check_control_preprocess(self, kind, canny_low=100, canny_high=200, canny_l2=False, blur_sigma=8.0, depth_resolution=518,
                                  depth_normalize="minmax", width=None, height=None):
        """the arguments of preprocess_control, refused by name before any work"""
        if kind not in CONTROL_PREPROCESSORS:
            raise ValueError(f"fluxmi: control_preprocess={kind!r}: expected one of {CONTROL_PREPROCESSORS} (a depth map comes from "
                             "\"depth_anything\", the Depth Anything estimator of config.depth_path; pose and the other maps that need weights are "
                             "not part of this project: pass the map itself)")
        if kind == "depth_anything":
            from modules import depth as da

            if getattr(self, "depth_model", None) is None:
                raise ValueError("fluxmi: control_preprocess=\"depth_anything\" needs the Depth Anything estimator: set config.depth_path to a local "
                                 "directory holding config.json and the weights of DepthAnythingForDepthEstimation (nothing is downloaded)")
            if isinstance(depth_resolution, bool) or not isinstance(depth_resolution, int) or not da.DEPTH_RES_MIN <= depth_resolution <= da.DEPTH_RES_MAX:
                raise ValueError(f"fluxmi: depth_resolution={depth_resolution!r}: expected an integer in {da.DEPTH_RES_MIN}..{da.DEPTH_RES_MAX} (the side "
                                 "the estimator sees, rounded to a multiple of 14)")
            if depth_normalize not in ops.DEPTH_NORMALIZE:
                raise ValueError(f"fluxmi: depth_normalize={depth_normalize!r}: expected one of {tuple(ops.DEPTH_NORMALIZE)}")
            if width is not None and height is not None:
                w, h = da.depth_input_size(int(width), int(height), depth_resolution)
                if (w // da.PATCH) * (h // da.PATCH) + 1 > da.MAX_TOKENS:
                    raise ValueError(f"fluxmi: depth_resolution={depth_resolution} on a {width} x {height} image is a {h // da.PATCH} x {w // da.PATCH} "
                                     f"patch grid, above the {da.MAX_TOKENS} tokens the estimator is checked at (74 x 74 + 1): lower depth_resolution")
        elif (depth_resolution, depth_normalize) != (518, "minmax"):
            raise ValueError("fluxmi: depth_resolution / depth_normalize belong to control_preprocess=\"depth_anything\"")
        try:
            ops.canny_thresholds(canny_low, canny_high)
        except ValueError as e:
            raise ValueError(f"fluxmi: canny_low={canny_low!r} / canny_high={canny_high!r}: expected integers >= 0 ({e})") from None
        if not isinstance(canny_l2, bool):
            raise ValueError(f"fluxmi: canny_l2={canny_l2!r}: expected a bool")
        try:
            ops.blur_radius(blur_sigma)
        except ValueError:
            raise ValueError(f"fluxmi: blur_sigma={blur_sigma!r}: expected a number whose radius ceil(3 sigma) lies in 1..{ops.BLUR_MAX_RADIUS}, "
                             f"i.e. 0 < blur_sigma <= {ops.BLUR_MAX_RADIUS / 3:.2f}") from None

    @torch.inference_mode()
    def preprocess_control(self, image, kind: str, width: Optional[int] = None, height: Optional[int] = None, canny_low: int = 100,
                           canny_high: int = 200, canny_l2: bool = False, blur_sigma: float = 8.0, depth_resolution: int = 518,
                           depth_normalize: str = "minmax") -> torch.Tensor:
        """A photo -> the control map a FLUX.1 Canny [dev] checkpoint or a ControlNet follows: uint8 [H, W, 3] on the host.  `image`: any form
        `init_image` takes.  It is first resized to (width, height) with PIL LANCZOS, exactly as prepare_control_conditioning resizes a map
        (BFL runs its Canny after the resize too; None keeps the image's own size), then goes to the autoencoder's device and through one
        of the kernels of csrc/preprocess.hip (fluxmi.ops):
          "canny"  edges 0 / 255 of the Canny detector defined in include/fluxmi.h: integer arithmetic, exact and deterministic.  It follows
                   the well-known algorithm, but parity with an OpenCV binary is NOT pinned (none is available to the tests).  The defaults
                   100 / 200 are the thresholds of diffusers' ControlNet examples; BFL's FLUX.1 Canny pipeline uses 50 / 200.  Those are
                   theirs -- no threshold is recommended here.  `canny_l2`: squared-gradient magnitudes (OpenCV's L2gradient).
          "gray"   PIL's convert("L"), bit for bit
          "blur"   a Gaussian blur of standard deviation `blur_sigma` pixels (radius ceil(3 sigma) <= 64), replicated border
          "depth_anything"  the depth map of the Depth Anything estimator of config.depth_path (modules/depth.py; near = bright): the resized
                   image goes through DPTImageProcessor's steps as the checkpoints configure them (PIL bicubic to the size of
                   modules.depth.depth_input_size for `depth_resolution` -- the side closer to it becomes it, both sides multiples of 14 --,
                   x / 255, ImageNet mean / std), the model, and fluxmi_depth_to_map back to the image's size: `depth_normalize` "minmax"
                   maps the image's own min..max to 0..255 (the form diffusers' and the ControlNet annotators' depth maps take), "raw"
                   writes clamp(depth, 0, 255).  Parity with BFL's DepthImageEncoder post-processing is NOT pinned.
        A one-channel result is repeated to three channels.  Pose, tile and low-quality maps are not made here."""
        from PIL import Image

        self._check_control_preprocess(kind, canny_low, canny_high, canny_l2, blur_sigma, depth_resolution, depth_normalize, width, height)
        pil = self._rgb_uint8(image).convert("RGB")
        size = (pil.width if width is None else int(width), pil.height if height is None else int(height))
        if size != pil.size:
            pil = pil.resize(size, Image.LANCZOS)
        if kind == "depth_anything":
            return self.depth_model.depth_map(pil, (size[1], size[0]), depth_resolution, depth_normalize).cpu()
        dev = self.device_ae if getattr(self, "ae", None) is not None else self.device_flux
        x = torch.from_numpy(np.array(pil)).to(dev)[None].contiguous()
        if kind == "canny":
            y = ops.canny(x, canny_low, canny_high, canny_l2)
        elif kind == "gray":
            y = ops.rgb_to_gray(x)
        else:
            y = ops.gaussian_blur(x, blur_sigma)
        y = y[0] if y.ndim == 4 else y[0][..., None].expand(-1, -1, 3)
        return y.contiguous().cpu()

    # ---- FLUX IP-Adapter image prompts ---------------------------------------------------------------------------------------------------
    def prepare_ip_adapter(self, images, image_embeds, scale, negative_image, negative_scale, guided: bool):
        """-> (call, guided_call): the `ip_adapter=` arguments of Flux.denoise for the unguided steps (the prompt branch's K / V, [depth, 1,
        Nk, H]) and, for a guided request, for the guided steps ([depth, 2, Nk, H]: prompt branch, then negative branch with its own K / V
        and scale; else None).  The negative branch defaults to black images, one per prompt image (XLabs); a float tensor [n, 768] is
        taken as embeds."""
        from modules.ip_adapter import IPAdapterCall

        ad = self.ip_adapter
        emb = ad.embed(images) if image_embeds is None else image_embeds
        k, v = ad.kv(emb)
        call = IPAdapterCall(k, v, scale)
        if not guided:
            return call, None
        if isinstance(negative_image, torch.Tensor) and negative_image.is_floating_point():
            nemb = negative_image
        else:
            n = emb.shape[0]
            if negative_image is None:
                S = ad.clip.cfg["image_size"] if ad.clip is not None else 224
                negative_image = [np.zeros((S, S, 3), dtype=np.uint8)] * n
            nemb = ad.embed(negative_image)
        if nemb.shape[0] != emb.shape[0]:
            raise ValueError(f"fluxmi: negative_ip_adapter_image holds {nemb.shape[0]} images, ip_adapter_image {emb.shape[0]} (both branches "
                             "run in one batch: the same number of image tokens)")
        nk, nv = ad.kv(nemb)
        return call, IPAdapterCall(torch.cat((k, nk), 1), torch.cat((v, nv), 1), torch.cat((scale, negative_scale), 0))

    # ---- FLUX.1 Redux image prompts ------------------------------------------------------------------------------------------------------
    def _require_redux(self):
        if self.redux is None:
            raise ValueError("fluxmi: redux_image needs the FLUX.1 Redux image encoder: set config.redux_path (flux1-redux-dev.safetensors) and "
                             "config.siglip_path (the SigLIP vision tower, a local HF directory or .safetensors file)")

    @staticmethod
    def _redux_list(redux_image) -> list:
        return list(redux_image) if isinstance(redux_image, (list, tuple)) else [redux_image]

    @torch.inference_mode()
    def prepare_redux_tokens(self, images, num_images: int = 1, txt: Optional[torch.Tensor] = None):
        """FLUX.1 Redux [dev]: steps 1-4 of modules/image_embedders.py's docstring.  `images`: one image in any form `init_image` takes,
        or a list of them (729 tokens per image, in list order).  Returns the Redux tokens [num_images, 729 n, 4096] in the flow dtype on
        the flow device; with `txt` [num_images, Lt5, 4096] (the T5 states), returns (txt, txt_ids) with the tokens appended behind the T5
        tokens and txt_ids = zeros [num_images, Lt5 + 729 n, 3], as BFL's prepare_redux builds them."""
        self._require_redux()
        tok = self.redux(self._redux_list(images)).to(device=self.device_flux, dtype=torch.bfloat16)
        tok = tok.reshape(1, -1, tok.shape[-1]).to(self.dtype).repeat(num_images, 1, 1)
        if txt is None:
            return tok
        txt = torch.cat((txt, tok.to(txt)), dim=-2)
        return txt, torch.zeros(txt.shape[0], txt.shape[1], 3, device=txt.device, dtype=txt.dtype)

    # ---- packing / ids (reference flux_pipeline.py:267-292, 440-448) ----------------------------------------------
    @staticmethod
    def pack(img: torch.Tensor) -> torch.Tensor:
        b, c, h, w = img.shape
        return img.reshape(b, c, h // 2, 2, w // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(b, (h // 2) * (w // 2), c * 4)

    def unpack(self, x: torch.Tensor, height: int, width: int) -> torch.Tensor:
        b = x.shape[0]
        h, w = math.ceil(height / 16), math.ceil(width / 16)
        return x.reshape(b, h, w, -1, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(b, -1, h * 2, w * 2)

    @staticmethod
    def make_img_ids(bs: int, h2: int, w2: int, device, dtype) -> torch.Tensor:
        ids = torch.zeros(h2, w2, 3, device=device, dtype=dtype)
        ids[..., 1] = ids[..., 1] + torch.arange(h2, device=device, dtype=dtype)[:, None]
        ids[..., 2] = ids[..., 2] + torch.arange(w2, device=device, dtype=dtype)[None, :]
        return ids[None].repeat(bs, 1, 1, 1).flatten(1, 2)

    @torch.inference_mode()
    def prepare(self, img: torch.Tensor, prompt, target_device=None, target_dtype=None):
        """-> img tokens, img_ids, vec, txt, txt_ids (reference flux_pipeline.py:234-312)."""
        target_device = self.device_flux if target_device is None else target_device
        target_dtype = self.dtype if target_dtype is None else target_dtype
        bs, c, h, w = img.shape
        tokens = self.pack(img)
        assert tokens.shape == (bs, (h // 2) * (w // 2), c * 4), f"{tokens.shape} != {(bs, (h // 2) * (w // 2), c * 4)}"
        prompts = None
        if isinstance(prompt, (list, tuple)):
            # reference flux_pipeline.py:267-278: a list with num_images == 1 sizes the batch by its length (the one noise sample is
            # repeated).  The reference then hands the LIST to parse_prompt_attention, whose regex scan raises TypeError; here every
            # prompt of the list is embedded on its own, which is what the batch sizing implies.
            if not prompt or not all(isinstance(q, str) for q in prompt):
                raise TypeError("fluxmi: a prompt list must be a non-empty list of str")
            prompts = list(prompt)
            if bs == 1 and len(prompts) > 1:
                bs = len(prompts)
                tokens = tokens.repeat_interleave(bs, dim=0)
            elif len(prompts) == 1:
                prompts = prompts * bs
            elif len(prompts) != bs:
                raise ValueError(f"fluxmi: {len(prompts)} prompts for a batch of {bs} images")
        img_ids = self.make_img_ids(bs, h // 2, w // 2, target_device, target_dtype)
        if isinstance(prompt, dict):
            txt = prompt["txt"].to(device=target_device, dtype=target_dtype)
            vec = prompt["vec"].to(device=target_device, dtype=target_dtype)
            if txt.shape[0] == 1 and bs > 1:
                txt, vec = txt.expand(bs, -1, -1), vec.expand(bs, -1)
        elif self.t5 is not None and self.clip is not None:
            from flux_emphasis import get_weighted_text_embeddings_flux

            kw = dict(device=self.device_clip, target_device=target_device, target_dtype=target_dtype, debug=self.debug)
            if prompts is not None:
                parts = [get_weighted_text_embeddings_flux(self, q, num_images_per_prompt=1, **kw) for q in prompts]
                vec, txt, txt_ids = (torch.cat([pt[i] for pt in parts], 0) for i in range(3))
                return tokens, img_ids, vec, txt, txt_ids
            if not isinstance(prompt, str):
                raise TypeError("fluxmi: prompt must be a str, a list of str, or a dict of pre-computed embeddings")
            vec, txt, txt_ids = get_weighted_text_embeddings_flux(self, prompt, num_images_per_prompt=bs, **kw)
            return tokens, img_ids, vec, txt, txt_ids
        else:
            raise RuntimeError("fluxmi: no text encoders attached (config.text_enc_path / clip_path not found). Pass "
                               "prompt={'txt': T5 states [B,Lt,4096], 'vec': CLIP pooled [B,768]} or load the encoders.")
        txt_ids = torch.zeros(bs, txt.shape[1], 3, device=target_device, dtype=target_dtype)
        return tokens, img_ids, vec, txt, txt_ids

    def _region_text(self, prompt) -> torch.Tensor:
        """T5 states [1, Lt, C] of one region prompt (prompt weighting syntax included), or the `txt` of pre-computed embeddings.  Only the
        text stream of a region is used (y and guidance come from the base prompt), so CLIP does not run and no image ids are built."""
        if isinstance(prompt, dict):
            return prompt["txt"].to(device=self.device_flux, dtype=self.dtype)
        if not isinstance(prompt, str):
            raise TypeError("fluxmi: a region prompt must be a str or a dict of pre-computed embeddings")
        if self.t5 is None or self.clip is None:
            raise RuntimeError("fluxmi: no text encoders attached; pass region prompts as {'txt': T5 states [1, Lt, C]}")
        from flux_emphasis import get_weighted_text_embeddings_flux

        return get_weighted_text_embeddings_flux(self, prompt, num_images_per_prompt=1, device=self.device_clip, target_device=self.device_flux,
                                                 target_dtype=self.dtype, debug=self.debug, need_clip=False)[1]

    def _prepare_negative(self, negative_prompt, noise: torch.Tensor, num_images: int, txt: torch.Tensor):
        """The negative prompt through prepare()'s text path (prompt weighting syntax included) -> (vec, txt) [num_images, ...] matching the
        prompt's `txt`.  Checked here, before any collective: every rank sees the same shapes, so every rank raises."""
        if isinstance(negative_prompt, (list, tuple)) and len(negative_prompt) not in (1, num_images):
            raise ValueError(f"fluxmi: {len(negative_prompt)} negative prompts for a batch of {num_images} images (one, or one per image)")
        _, _, neg_vec, neg_txt, _ = self.prepare(noise[:1].expand(num_images, -1, -1, -1), negative_prompt)
        if tuple(neg_txt.shape[1:]) != tuple(txt.shape[1:]) or neg_txt.shape[0] not in (1, num_images):
            raise ValueError(f"fluxmi: negative_prompt embeddings {tuple(neg_txt.shape)} do not match the prompt's {tuple(txt.shape)}: both branches "
                             "run in one batch and need the same sequence length")
        return neg_vec.expand(num_images, -1).contiguous(), neg_txt.expand(num_images, -1, -1).contiguous()

    # ---- LoRA (reference flux_pipeline.py:151-177) -------------------------------------------------------------------
    def load_lora(self, lora_path, scale: float, name: Optional[str] = None):
        self.model.load_lora(path=lora_path, scale=scale, name=name)

    def unload_lora(self, path_or_identifier: str):
        self.model.unload_lora(path_or_identifier=path_or_identifier)

    # ---- calibration warm-up (the part of reference compile() that matters, flux_pipeline.py:197-212) -----------------
    @torch.inference_mode()
    def compile(self, prompt=None):
        if self.config.prequantized_flow:
            return
        p = self.model.params
        lt = self.config.text_enc_max_length
        if prompt is None:
            if self.t5 is not None and self.clip is not None:
                # the reference's own warm-up prompt (flux_pipeline.py:199): the frozen input scales then reflect real text activations
                prompt = "A beautiful test image used to solidify the fp8 nn.Linear input scales prior to compilation 😉"
            else:
                # no encoders attached (offline runs): synthetic embeddings of T5 / CLIP-like statistics.  The scales are then tuned on
                # noise-like conditioning -- callers with real embeddings should pass them as `prompt`
                g = torch.Generator().manual_seed(10)
                prompt = {"txt": 0.1 * torch.randn(1, lt, p.context_in_dim, generator=g), "vec": torch.randn(1, p.vec_in_dim, generator=g)}
        # batch-sharded replicas: every layer's running amax is MAX-reduced across the ranks inside each calibrating step, so all
        # replicas freeze the SAME input scales (float8_quantize.py:227 takes amax over the whole batch)
        world = fdist.world_size()
        if world > 1:
            self.model.enable_amax_exchange()
        kw = dict(prompt=prompt, height=768, width=768, num_steps=12, guidance=3.5, seed=10, silent=True, output_type="latent",
                  num_images=max(1, world))
        kw.update(self._warmup_conditioning(768, 768))
        if self.name == ModelVersion.flux_schnell.value or self.name == "flux-schnell":
            kw["num_steps"] = 4
            for _ in range(3):
                self.generate(**kw)
        else:
            self.generate(**kw)
            self.generate(**{**kw, "num_steps": 1})  # 13th call: freezes the input scales
        if world > 1:
            self.model.enable_amax_exchange(False)
        if getattr(self, "controlnet", None) is not None:
            # the ControlNet calibrates on its own counter (the main model's scales are frozen by now): the same 13 calls with a mid-grey
            # control image through the autoencoder, or N(0, 1) control latents without one
            ckw = dict(control_mode=0) if self.controlnet.is_union else {}
            if self.ae is not None and getattr(self.ae, "encoder_loaded", True):
                ckw["controlnet_image"] = np.full((kw["height"], kw["width"], 3), 128, dtype=np.uint8)
            else:
                g = torch.Generator().manual_seed(11)
                ckw["controlnet_cond"] = torch.randn(1, (kw["height"] // 16) * (kw["width"] // 16), p.in_channels, generator=g)
            for n in ((4, 4, 4, 1) if kw["num_steps"] == 4 else (12, 1)):
                self.generate(**{**kw, **ckw, "num_steps": n})
        if self.redux is not None:
            # one Redux request on the frozen scales, so that the encoder and the longer text stream have run before serving
            self.generate(**{**kw, "num_steps": 1, "redux_image": np.full((384, 384, 3), 128, dtype=np.uint8)})

    def _warmup_conditioning(self, height: int, width: int) -> dict:
        """compile()'s conditioning for a Fill / Depth / Canny model, so that img_in sees its real width and (fp8 embedders) its input scale
        covers the conditioning channels: a mid-grey image and a centred rectangular mask (Fill) or a mid-grey control image through the
        autoencoder; without one, N(0, 1) latents and the same mask, packed.  Nothing for a text-to-image model."""
        kind = self.conditioning_kind()
        if kind is None:
            return {}
        mask = np.zeros((height, width), dtype=np.uint8)
        mask[height // 4:height - height // 4, width // 4:width - width // 4] = 255
        grey = np.full((height, width, 3), 128, dtype=np.uint8)
        if self.ae is not None:
            return dict(init_image=grey, mask_image=mask) if kind == "fill" else dict(control_image=grey)
        z = torch.randn(1, 16, height // 8, width // 8, generator=torch.Generator().manual_seed(11)).to(torch.bfloat16)
        cond = self.pack(z)
        if kind == "fill":
            cond = torch.cat((cond, self.pack_fill_mask(torch.from_numpy(mask).float().div(255.0)[None, None])), -1)
        return dict(img_cond=cond)

    # ---- the request (reference flux_pipeline.py:526-663) ---------------------------------------------------------------
    @torch.inference_mode()
    def generate(self, prompt, width: int = 720, height: int = 1024, num_steps: int = 24, guidance: float = 3.5,
                 seed: int | None = None, init_image=None, strength: float = 1.0, silent: bool = False, num_images: int = 1,
                 return_seed: bool = False, jpeg_quality: int = 99, output_type: str = "jpeg", noise: Optional[torch.Tensor] = None,
                 use_graph: bool = True, reference_image=None, mask_image=None, control_image=None,
                 img_cond: Optional[torch.Tensor] = None, redux_image=None, negative_prompt=None, true_cfg_scale: float = 1.0,
                 true_cfg_interval=(0.0, 1.0), cache_threshold: float = 0.0, cache_max_hits: int = 0, regions=None,
                 regional_tokens: int = 128, inpaint_mask=None, inpaint_differential: bool = False, controlnet_image=None,
                 controlnet_conditioning_scale: float = 1.0, control_mode: Optional[int] = None, control_guidance_start: float = 0.0,
                 control_guidance_end: float = 1.0, controlnet_cond: Optional[torch.Tensor] = None, sampler: str = "euler",
                 sigma_schedule: Optional[str] = None, sigmas=None, eta: float = 1.0, s_noise: float = 1.0, noise_seed: Optional[int] = None,
                 ip_adapter_image=None, ip_adapter_image_embeds: Optional[torch.Tensor] = None, ip_adapter_scale=1.0,
                 negative_ip_adapter_image=None, negative_ip_adapter_scale=1.0, guidance_mode: str = "cfg", guidance_rescale: float = 0.0,
                 apg_eta: float = 1.0, apg_norm_threshold: float = 0.0, apg_momentum: float = 0.0, zero_init_steps: int = 0,
                 on_step=None, preview_every: int = 0, preview_factors=None, source_prompt=None, source_guidance: Optional[float] = None,
                 edit_n_max: Optional[int] = None, edit_n_min: int = 0, edit_n_avg: int = 1, tile_size=None, tile_overlap: Optional[int] = None,
                 tile_weight: str = "cosine", upscale: bool = False, init_upscale: bool = False, control_preprocess: Optional[str] = None,
                 canny_low: int = 100, canny_high: int = 200, canny_l2: bool = False, blur_sigma: float = 8.0, depth_resolution: int = 518,
                 depth_normalize: str = "minmax", jpeg_encoder: Optional[str] = None):
        """`reference_image` (FLUX.1 Kontext [dev] instruction editing): an image the prompt describes an edit of, in any form `init_image`
        takes; see prepare_kontext_reference.  Composes with `init_image` / `strength` unchanged.
        FLUX.1 Fill [dev] (a model with 320 conditioning channels): `init_image` is the image to inpaint and `mask_image` (white =
        regenerate) is required; see prepare_fill_conditioning.  At strength 1.0 (BFL's only mode) the generation starts from pure noise;
        strength < 1 also blends the VAE latents of `init_image` into the start as img2img does.  BFL recommends guidance 30, ~50 steps.
        FLUX.1 Depth / Canny [dev] (64 conditioning channels): `control_image` (the depth map or edge map) is required; see
        prepare_control_conditioning.  Both take any form `init_image` takes.  `img_cond`: the conditioning tokens [1 or num_images, Li,
        in_channels - out_channels] already prepared (instead of `mask_image` / `control_image`).  A text-to-image model refuses all three.
        `redux_image` (FLUX.1 Redux [dev] image prompt; needs config.redux_path / siglip_path): an image in any form `init_image` takes, or a
        list; 729 SigLIP-derived tokens per image are appended to the T5 tokens (see prepare_redux_tokens).  It only lengthens the text
        stream, so it composes with everything above.
        `negative_prompt` + `true_cfg_scale` (the names of diffusers' FluxPipeline): true classifier-free guidance.  It runs iff
        `negative_prompt is not None and true_cfg_scale > 1`: every guided step predicts the prompt and the negative prompt in one forward
        on twice the batch and steps the latent with `neg + true_cfg_scale * (pos - neg)` (Flux.denoise), which costs about what twice
        the images cost.  A negative prompt with a scale <= 1 is ignored (not even encoded); a scale > 1 without one is refused.
        `negative_prompt` takes what `prompt` takes: a str ("" is valid), a list of one entry or one per image, or a dict of embeddings
        with the prompt's sequence length.  `guidance` (the distilled embedding) is independent of it and goes to both branches, as do a
        Kontext reference, Fill / Depth / Canny conditioning and `init_image` / `strength`; Redux tokens are appended to BOTH branches,
        so the guidance then acts on the text alone.  A seed draws the same noise with and without a negative prompt.
        `true_cfg_interval=(lo, hi)`, fractions of the request's n steps: step i (0-based) is guided iff lo n <= i < hi n, the others run
        the prompt alone.  Run as up to three consecutive denoise calls on slices of the schedule; the engine keeps one workspace and one
        graph, so every switch re-allocates and re-captures (README: measured).
        `cache_threshold` > 0 (+ `cache_max_hits`): first-block step caching (Flux.denoise; diffusers' FirstBlockCacheConfig): a frozen step
        whose first double block's residual moved by less than the threshold since the last full step skips every later block and reuses
        that step's residual.  Off by default; an approximation when on -- no threshold is recommended here (README).  Each of the up to
        three denoise calls of a `true_cfg_interval` request starts with an empty cache.
        `regions` (regional prompts): a list of {"prompt": ..., "box": (x0, y0, x1, y1)} (0..1 of the image) or {"prompt": ..., "mask": image}
        entries.  Rows [0, regional_tokens) of each region prompt's T5 states are appended to the text stream (behind the prompt's and any
        Redux tokens; `y` and `guidance` stay the base prompt's, txt_ids stay zero) and every attention runs under the token-group mask of
        build_region_groups: a region's text and the image tokens it covers see each other, the base prompt sees and is seen by every
        image token, image tokens see all image tokens.  `regional_tokens` is a multiple of 16.  Composes with img2img, a Kontext
        reference (its rows count as uncovered), Fill / Depth / Canny, Redux, LoRA, step caching and a negative prompt (the negative
        branch carries the same rows, masked out of every other token's view).  Under a process group the region text rides in the one
        request broadcast; the table is a pure function of the request's arguments, the same on every rank.  Without `regions` nothing
        changes, the text-encoder calls included.
        `inpaint_mask` (masked-latent inpainting; diffusers' FluxInpaintPipeline, on a Kontext / Depth / Canny model its Kontext / Control
        counterparts): white = regenerate, black = keep `init_image`, which is required; see prepare_inpaint_mask.  Works with the model
        that is loaded, no Fill checkpoint needed: after every step the kept part of the latent is replaced by the init latent noised to
        the step's time (Flux.denoise), so the kept latent pixels of the result are the encoded `init_image` exactly.  A new keyword on
        purpose: `mask_image` stays FLUX.1 Fill's conditioning; on a Fill model `inpaint_mask` is a hard composite on top of it.
        `inpaint_differential=True` (differential diffusion): the mask is a grey change map, released step by step (inpaint_thresholds).
        Composes with strength, `noise=`, num_images, a Kontext reference (noisy rows only), Depth / Canny, Redux, regions, step caching, a
        negative prompt and LoRA.  Image quality on real FLUX weights is not established here.
        `controlnet_image` (a FLUX ControlNet, config.controlnet_path: a diffusers-format FluxControlNetModel checkpoint): the edge map, depth
        map, pose ... to follow, in any form `init_image` takes (prepare_controlnet_conditioning), or `controlnet_cond`, its packed latents
        [1 or num_images, Li, 64] already prepared.  `controlnet_conditioning_scale` (any float) scales the net's residuals; a Union net needs
        `control_mode`; `control_guidance_start` / `control_guidance_end` follow diffusers: step i of n is controlled iff not (i / n < start
        or (i + 1) / n > end) -- run as consecutive denoise calls on slices of the schedule, like `true_cfg_interval`.  Composes with img2img,
        num_images, `noise=`, LoRA on the main model, Redux (the net sees the same text rows), a negative prompt (both branches are
        controlled) and `inpaint_mask`; refused with `regions`, `cache_threshold` > 0, `reference_image` and a Fill / Depth / Canny model.
        Without it the request is today's, launch for launch.
        `sampler`: "euler" (the default: today's kernels, launch for launch), "heun" (diffusers' FlowMatchHeunDiscreteScheduler: two model
        evaluations per step but the last), "midpoint" (RK2, two evaluations per step), "ab2" (Adams-Bashforth 2, one evaluation per step)
        or "dpmpp_2m" (DPM-Solver++(2M), one evaluation per step); see fluxmi.solvers.  `sigmas` (diffusers' argument): the request's own
        descending list in (0, 1], with or without a trailing 0, instead of get_schedule's -- `num_steps` then follows its length.
        `sigma_schedule`: "karras" (rho 7) or "exponential" re-spaces the schedule between its first and last non-zero value.  The program is
        built from the final timestep list, after the `strength` truncation; where `true_cfg_interval` or the control guidance interval
        cuts the request into several denoise calls, each call gets the program of its own slice (a multistep solver restarts with a
        first-order step there).  Composes with everything above except `cache_threshold` > 0, which a non-Euler sampler refuses.  Image
        quality per sampler on real FLUX weights is not established here; no sampler or step count is recommended.
        Stochastic samplers: `sampler` "euler_ancestral" (k-diffusion's rectified-flow ancestral step) or "dpmpp_2m_sde"
        (SDE-DPM-Solver++(2M)), one evaluation per step, with `eta` in [0, 1] (the share of each step's noise that is re-drawn; 0 = the
        deterministic limit) and `s_noise` >= 0 (a factor on the drawn noise).  The fresh noise is generated inside the update kernel by a
        counter-based generator (fluxmi.solvers; fluxmi_philox_normal): image k of the request draws under ids (seed & 0xffffffff,
        seed >> 32, k, 0), `seed` being `noise_seed` if given, else the request's seed (the integer set_seed returns; with several ranks
        and no seed given that is each rank's own), at the evaluation's index within the whole request: a request cut by
        `true_cfg_interval` or the control guidance interval never reuses a draw, and nothing is taken from the request's torch generator.
        A request or slice whose program draws nothing (eta 0, s_noise 0, the lone step onto sigma 0) runs as a deterministic solver call.
        Composes like the other samplers; `eta`, `s_noise` or `noise_seed` with a deterministic sampler is refused.
        `ip_adapter_image` (a FLUX IP-Adapter in the XLabs format, config.ip_adapter_path + clip_vision_path; modules/ip_adapter.py): an
        image prompt in any form `init_image` takes, or a list -- several images concatenate their tokens (Nk = T n <= 64; an extension of
        XLabs, as the image list is for Redux) -- or `ip_adapter_image_embeds`, the CLIP image_embeds [n, 768] already computed (the tower is
        skipped).  Unlike Redux it does not lengthen the text stream: every double block adds `ip_adapter_scale` (a float, or one float
        per double block) times a small cross-attention of its image queries over the image tokens.  With a negative prompt the negative
        branch gets `negative_ip_adapter_image` (default: a black image, as XLabs does; the same number of images; a [n, 768] tensor is
        taken as embeds) at `negative_ip_adapter_scale`.  Composes with img2img, num_images, LoRA, Redux, a Kontext reference, Fill /
        Depth / Canny, a negative prompt, `inpaint_mask`, every sampler and a ControlNet; refused with `regions`, `cache_threshold` > 0 and
        under a process group.  Parity with XLabs' code is unpinned and image quality on real weights is not established here (README).
        Without it the request is today's, launch for launch.
        Guidance shaping of true CFG (a guided request only; Flux.denoise `guidance_shaping`, csrc/guidance.hip): `guidance_mode` "cfg" (the
        default), "apg" (adaptive projected guidance, Sadat et al. 2024: the guidance difference is split along the prompt prediction,
        `apg_eta` scales the parallel part, `apg_norm_threshold` > 0 clips the difference's norm, `apg_momentum` (usually negative) keeps a
        running difference) or "cfg_zero_star" (Fan et al. 2025: the negative branch is rescaled by the optimised s* = <c, u> / <u, u>);
        `guidance_rescale` in [0, 1] (Lin et al. 2023 section 3.4; diffusers' name) pulls the guided prediction's standard deviation back
        to the prompt branch's; `zero_init_steps` replaces the prediction of the request's first k model EVALUATIONS by zero (CFG-Zero*'s
        zero-init; Heun and midpoint evaluate twice per step, and an evaluation outside `true_cfg_interval` counts but is never zeroed).
        Shaping runs iff the request is guided and (guidance_mode != "cfg" or guidance_rescale > 0 or zero_init_steps > 0): two more
        launches per evaluation, statistics per image; otherwise the request is today's, launch for launch.  Any non-default value
        without guidance (no negative prompt, or true_cfg_scale <= 1) is refused.  APG's running difference starts at 0 in front of every
        guided denoise call (one per request unless a ControlNet interval cuts the guided slice) and advances once per evaluation.
        Composes with everything a negative prompt composes with, step caching included.  Parity with diffusers' code is unpinned (the
        formulas of include/fluxmi.h are the definition) and image quality on real FLUX weights is NOT established here.
        `on_step(info)`: progress, live previews and cancellation.  Called once per model evaluation, in order, from this thread, behind the
        GPU's work on that evaluation, with info = {"evaluation", "num_evaluations", "step", "preview"}: `step` is the request's step the
        evaluation belongs to (a sampler's step_of_eval; Heun and midpoint evaluate twice per step) and `preview` a uint8 array
        [num_images, height / 8, width / 8, 3] -- the denoised estimate x - t v of that evaluation projected 16 -> 3 by one more launch in
        front of the update (csrc/preview.hip) -- at the evaluations with evaluation % preview_every == 0, None elsewhere (always None
        with preview_every = 0).  The numbering continues across the denoise calls `true_cfg_interval` or a ControlNet interval cuts the
        request into.  Returning False cancels: the engine stops launching (at most two evaluations run on), and generate raises
        fluxmi.GenerationCancelled, which carries the evaluations run; an exception raised in on_step surfaces here the same way.
        `preview_factors` = ([16][3], [3]) in decoded-latent space; default: the config's preview_factors / preview_bias, else a least-squares
        fit against this pipeline's VAE, made on first use and cached (util.fit_preview_factors).  preview_every > 0 without on_step is
        refused, both are refused under a process group and for more images than one engine pass holds.  Without them the request is
        today's, launch for launch.  Composes with everything else.
        `source_prompt` (FlowEdit, Kulikov et al. 2024: inversion-free text-guided editing on a plain text-to-image checkpoint): a prompt
        that DESCRIBES `init_image`, in any form `prompt` takes and of its sequence length; `prompt` is then the target prompt and the
        result is `init_image` under it -- no mask, no extra weights, no inversion pass.  It runs iff `source_prompt is not None` and needs
        `init_image`, strength 1.0 and sampler "euler".  Of the request's `num_steps` steps the last `edit_n_max` (None = all) are edited;
        the last `edit_n_min` of those are a plain Euler tail on the target prompt (0 = none), the others are coupled steps: `edit_n_avg`
        model evaluations each, on both prompts at once (one forward on two samples per image; Flux.denoise_edit, fluxmi.flowedit).
        `guidance` is the target branch's distilled guidance, `source_guidance` the source branch's (None = `guidance`).  The noise of
        the couplings is generated in the update kernel from `noise_seed` (None = the request's seed): nothing is drawn from the request's
        torch generator, and image k of the request draws under ids (seed & 0xffffffff, seed >> 32, k, 1).  Composes with LoRA,
        `num_images` (at most 16), `sigmas` / `sigma_schedule` and `on_step` (progress and cancellation; no previews); refused with a
        negative prompt at a scale > 1, `inpaint_mask`, `reference_image`, a Fill / Depth / Canny model, `regions`, `cache_threshold` > 0,
        a ControlNet, an IP-Adapter, `redux_image`, `preview_every` > 0 and under a process group.  Without `source_prompt` the request is
        today's, launch for launch, and `source_guidance` / `edit_*` are refused.
        `tile_size` (tiled generation; MultiDiffusion, Bar-Tal et al. 2023, known as tiled diffusion): an int (a square window) or (height,
        width) in pixels, multiples of 16, at most the request's size.  The request's latent is then one large canvas and every step runs
        the model on overlapping windows of that size -- each a stand-alone image to the model, all of them samples of one engine batch --
        blends their predictions where they overlap (`tile_weight`: "cosine", a Hann profile over the window, or "uniform") and steps the
        canvas once (Flux.denoise_windows, fluxmi.windows, csrc/window_step.hip): cost linear in area.  `tile_overlap` in pixels, a multiple
        of 16 with 0 <= overlap < tile, is the overlap of neighbouring windows (None: a quarter of the tile, rounded down to a multiple of
        16); the last window of an axis snaps to the canvas edge.  Noise is drawn at canvas size from the request's generator, `init_image`
        / `strength` run at canvas size as for any request (img2img upscaling), the schedule's shift follows the WINDOW's sequence length,
        text and `y` are shared by all windows, and the result is decoded at canvas size by the same VAE -- whose mid-block attention is
        quadratic in the canvas: beyond 46340 latent pixels (about 1720 x 1720 px) a request that decodes or encodes is refused, and
        output_type="latent" is what remains.  Composes with a negative prompt at `true_cfg_scale` > 1 (unshaped), `true_cfg_interval`,
        `init_image` / `strength`, LoRA, `num_images`, `sigmas` / `sigma_schedule`, `noise=` and `on_step` with preview_every = 0, while
        num_images x windows (twice that when guided) fit one engine pass of 32 samples.  Refused with any sampler but "euler", guidance
        shaping, `inpaint_mask`, `reference_image`, a Fill / Depth / Canny model, `redux_image`, `regions`, `cache_threshold` > 0, a
        ControlNet, an IP-Adapter, `source_prompt`, `preview_every` > 0 and under a process group.  `tile_size=None`, or a tile of the
        request's size with no other tile argument, is today's request, launch for launch; `tile_overlap` / `tile_weight` without
        `tile_size` are refused.  Image quality on real FLUX weights is not established here; no tile size or overlap is recommended.
        `upscale` / `init_upscale` (an ESRGAN-family RRDBNet, config.upscaler_path; modules/upscaler.py, FluxPipeline.upscale): with
        `upscale=True` the request's uint8 pixels go through the network before they are returned or JPEG-encoded, so the result is
        `upscaler.scale` times `width` x `height` -- for every request kind that returns pixels, tiled and FlowEdit ones included; with
        `init_upscale=True` `init_image` goes through it before the resize to `width` x `height` that the request already does, e.g.
        generate(prompt, init_image=photo, init_upscale=True, width=4096, height=4096, strength=0.3, tile_size=1024) on a
        vae_attention="streaming" config.  Refused up front: either flag without a configured upscaler, `upscale` with
        output_type="latent" (or no VAE), `init_upscale` without `init_image`, an image the network's kernel or the device's free memory
        cannot take.  Both False (the default) is today's request, launch for launch.
        `control_preprocess` ("canny" | "gray" | "blur" | "depth_anything"; preprocess_control): `control_image` (FLUX.1 Depth / Canny) or `controlnet_image` (a
        ControlNet) -- whichever the request carries -- is a PHOTO, and the control map is made from it on the device, after the resize to
        `width` x `height`, by a native Canny edge detector (`canny_low` / `canny_high` / `canny_l2`), PIL's luma, or a Gaussian blur
        (`blur_sigma`); the conditioning call then sees a correctly sized map.  The Canny is the integer definition of include/fluxmi.h:
        exact and deterministic, but parity with OpenCV's binary is unpinned.  100 / 200 are diffusers' example thresholds, BFL's
        pipeline uses 50 / 200; neither is a recommendation.  Refused up front: `control_preprocess` without `control_image` /
        `controlnet_image`, with `img_cond` / `controlnet_cond` (already-encoded maps), an unknown kind, thresholds that are not integers
        >= 0, a `blur_sigma` whose radius ceil(3 sigma) is outside 1..64.  None (the default) is today's request, launch for launch, and
        then refuses non-default `canny_*` / `blur_sigma`.
        `control_preprocess="depth_anything"` (+ `depth_resolution`, `depth_normalize`): the map is the depth map of the Depth Anything
        estimator of config.depth_path (modules/depth.py; preprocess_control has the steps), e.g. generate(prompt, control_image=photo,
        control_preprocess="depth_anything") on a FLUX.1 Depth [dev] model, or the same on `controlnet_image` with a Union ControlNet's depth
        mode.  `depth_resolution` (default 518, DPTImageProcessor's) is the side the estimator sees, `depth_normalize` "minmax" (default) or
        "raw".  Refused up front: the kind without a depth model (naming `depth_path`), a `depth_resolution` outside 14..1036, a patch grid
        above 74 x 74 + 1 tokens (the longest sequence the estimator's attention is checked at), an unknown `depth_normalize`, and either
        argument without the kind.  `control_preprocess="depth"` stays refused: the kind is named after its model.
        `jpeg_encoder` ("pil" | "native"; None = config.jpeg_encoder, "pil" unless configured): who writes the JPEG of output_type="jpeg".
        "pil" is today's path, byte for byte: pixels to the host, Pillow at `jpeg_quality`.  "native" keeps the pixels on the device from the
        VAE (and the upscaler) to fluxmi.ops.jpeg_encode -- a baseline JFIF file, 4:2:0, the Annex K tables at `jpeg_quality`, restart markers
        every 4 MCUs: libjpeg's integer pipeline (include/fluxmi.h), so it decodes to the pixels Pillow's file decodes to; the bytes differ
        only by the restart markers -- and two copies come back, the length and that many bytes.  It serves the plain, the tiled and the
        FlowEdit request and into_bytes; with another output_type it is ignored.  Refused by name: an unknown encoder, and with "native" a
        `jpeg_quality` outside 1..100 or an image beyond 65535 x 65535 (num_images stack vertically)."""
        if control_preprocess is not None:
            if img_cond is not None or controlnet_cond is not None:
                raise ValueError("fluxmi: control_preprocess works on an image: it does not combine with img_cond / controlnet_cond (maps that "
                                 "are already encoded)")
            if control_image is None and controlnet_image is None:
                raise ValueError("fluxmi: control_preprocess needs control_image (FLUX.1 Depth / Canny) or controlnet_image (a ControlNet): "
                                 "the photo to make the map from")
            self._check_control_preprocess(control_preprocess, canny_low, canny_high, canny_l2, blur_sigma, depth_resolution, depth_normalize,
                                           width, height)
        elif (canny_low, canny_high, canny_l2, blur_sigma) != (100, 200, False, 8.0):
            raise ValueError("fluxmi: canny_low / canny_high / canny_l2 / blur_sigma belong to control_preprocess, which is not set")
        elif (depth_resolution, depth_normalize) != (518, "minmax"):
            raise ValueError("fluxmi: depth_resolution / depth_normalize belong to control_preprocess=\"depth_anything\", which is not set")
        prep_kw = dict(canny_low=canny_low, canny_high=canny_high, canny_l2=canny_l2, blur_sigma=blur_sigma)
        if control_preprocess == "depth_anything":  # the other kinds keep the call they always made
            prep_kw.update(depth_resolution=depth_resolution, depth_normalize=depth_normalize)
        if upscale or init_upscale:
            init_image = self._check_upscale(upscale, init_upscale, output_type, init_image, width, height, num_images)
        jpeg_encoder = self._jpeg_encoder(jpeg_encoder)
        if jpeg_encoder == "native" and output_type == "jpeg" and self.ae is not None:
            up = self.upscaler.scale if upscale else 1
            self._check_jpeg_native(num_images, up * 16 * (height // 16), up * 16 * (width // 16), jpeg_quality)
        tiles = self._check_tiles(locals())
        if tiles is not None:
            return self._generate_tiled(tiles, prompt, width, height, num_steps, guidance, seed, init_image, strength, num_images, return_seed,
                                        jpeg_quality, output_type, noise, use_graph, negative_prompt, true_cfg_scale, true_cfg_interval,
                                        sigma_schedule, sigmas, on_step, upscale=upscale, jpeg_encoder=jpeg_encoder)
        edit = self._check_edit(locals())
        if edit is not None:
            return self._generate_edit(edit, prompt, source_prompt, width, height, num_steps, guidance, seed, init_image, silent, num_images,
                                       return_seed, jpeg_quality, output_type, use_graph, sigma_schedule, sigmas, noise_seed, on_step,
                                       upscale=upscale, jpeg_encoder=jpeg_encoder)
        if isinstance(preview_every, bool) or not isinstance(preview_every, int) or preview_every < 0:
            raise ValueError(f"fluxmi: preview_every={preview_every!r}: expected an integer >= 0 (0 = no previews)")
        if on_step is not None and not callable(on_step):
            raise ValueError("fluxmi: on_step must be callable")
        if preview_every > 0 and on_step is None:
            raise ValueError("fluxmi: preview_every > 0 needs on_step (the callback that receives the previews)")
        if preview_factors is not None and preview_every == 0:
            raise ValueError("fluxmi: preview_factors given with preview_every = 0")
        if on_step is not None and fdist.world_size() > 1:
            raise ValueError("fluxmi: on_step / preview_every are refused under a process group (the per-evaluation host waits would stall its "
                             "collectives)")
        preview_proj = self.preview_projection(preview_factors) if preview_every > 0 else None
        if guidance_mode not in GUIDANCE_MODES:
            raise ValueError(f"fluxmi: guidance_mode={guidance_mode!r}: expected one of {GUIDANCE_MODES}")
        try:
            guidance_rescale, apg_eta, apg_norm_threshold, apg_momentum = (float(v) for v in (guidance_rescale, apg_eta, apg_norm_threshold, apg_momentum))
            if isinstance(zero_init_steps, bool) or int(zero_init_steps) != zero_init_steps:
                raise ValueError
            zero_init_steps = int(zero_init_steps)
        except (TypeError, ValueError):
            raise ValueError("fluxmi: guidance_rescale / apg_eta / apg_norm_threshold / apg_momentum take floats, zero_init_steps an integer") from None
        if not all(math.isfinite(v) for v in (guidance_rescale, apg_eta, apg_norm_threshold, apg_momentum)):
            raise ValueError("fluxmi: guidance_rescale / apg_eta / apg_norm_threshold / apg_momentum must be finite")
        if not 0.0 <= guidance_rescale <= 1.0:
            raise ValueError(f"fluxmi: guidance_rescale={guidance_rescale}: expected a value in [0, 1]")
        if apg_norm_threshold < 0 or zero_init_steps < 0:
            raise ValueError(f"fluxmi: apg_norm_threshold={apg_norm_threshold} and zero_init_steps={zero_init_steps} must be >= 0")
        shaping_asked = (guidance_mode != "cfg" or guidance_rescale > 0 or zero_init_steps > 0 or apg_eta != 1.0 or apg_norm_threshold != 0.0
                         or apg_momentum != 0.0)
        if shaping_asked and not (negative_prompt is not None and true_cfg_scale > 1):
            raise ValueError("fluxmi: guidance_mode / guidance_rescale / apg_* / zero_init_steps shape true classifier-free guidance: they need a "
                             "negative_prompt and true_cfg_scale > 1")
        if guidance_mode != "apg" and (apg_eta != 1.0 or apg_norm_threshold != 0.0 or apg_momentum != 0.0):
            raise ValueError(f"fluxmi: apg_eta / apg_norm_threshold / apg_momentum belong to guidance_mode=\"apg\", not {guidance_mode!r}")
        shaping = None
        if guidance_mode != "cfg" or guidance_rescale > 0 or zero_init_steps > 0:
            shaping = dict(mode=guidance_mode, rescale=guidance_rescale, eta=apg_eta, norm_threshold=apg_norm_threshold, momentum=apg_momentum,
                           zero_init_steps=zero_init_steps)
        stochastic = sampler in solvers.STOCHASTIC_SAMPLERS
        if sampler not in solvers.SAMPLERS and not stochastic:
            raise ValueError(f"fluxmi: sampler={sampler!r}: expected one of {solvers.SAMPLERS + solvers.STOCHASTIC_SAMPLERS}")
        if not stochastic and (eta != 1.0 or s_noise != 1.0 or noise_seed is not None):
            raise ValueError(f"fluxmi: eta / s_noise / noise_seed shape the noise of a stochastic sampler {solvers.STOCHASTIC_SAMPLERS}; "
                             f"sampler={sampler!r} draws none")
        if stochastic:
            solvers.build_program(sampler, (1.0, 0.0), eta, s_noise)  # eta / s_noise out of range: refused before any work
            if noise_seed is not None and (isinstance(noise_seed, bool) or not isinstance(noise_seed, int) or not 0 <= noise_seed < 2 ** 64):
                raise ValueError(f"fluxmi: noise_seed={noise_seed!r}: expected an integer in [0, 2^64)")
        if sigma_schedule not in solvers.SIGMA_SCHEDULES:
            raise ValueError(f"fluxmi: sigma_schedule={sigma_schedule!r}: expected one of {solvers.SIGMA_SCHEDULES}")
        if sigmas is not None:
            sigmas = solvers.custom_sigmas(sigmas)
        try:
            cache_on = float(cache_threshold) > 0
        except (TypeError, ValueError):
            cache_on = False  # (refused below, with its own message)
        if sampler != "euler" and cache_on:
            raise ValueError(f"fluxmi: sampler={sampler!r} does not combine with cache_threshold > 0 (the step cache compares consecutive "
                             "evaluations; a solver may evaluate one time twice)")
        sched_kw = {k: v for k, v in (("sigmas", sigmas), ("sigma_schedule", sigma_schedule)) if v is not None}
        cn_on = controlnet_image is not None or controlnet_cond is not None
        if cn_on:
            if getattr(self, "controlnet", None) is None:
                raise ValueError("fluxmi: controlnet_image needs a ControlNet: set config.controlnet_path (a local diffusers-format "
                                 "FluxControlNetModel checkpoint)")
            if controlnet_image is not None and controlnet_cond is not None:
                raise ValueError("fluxmi: pass controlnet_image or controlnet_cond, not both")
            if regions is not None:
                raise ValueError("fluxmi: regions do not combine with a ControlNet")
            if float(cache_threshold) > 0:
                raise ValueError("fluxmi: cache_threshold > 0 (step caching) does not combine with a ControlNet")
            if reference_image is not None:
                raise ValueError("fluxmi: a Kontext reference_image does not combine with a ControlNet")
            if self.conditioning_kind() is not None:
                raise ValueError("fluxmi: a FLUX.1 Fill / Depth / Canny model takes no ControlNet")
            if self.controlnet.is_union and control_mode is None:
                raise ValueError(f"fluxmi: a Union ControlNet needs control_mode (0..{self.controlnet.num_mode - 1})")
            if self.controlnet.is_union and not 0 <= int(control_mode) < self.controlnet.num_mode:
                raise ValueError(f"fluxmi: control_mode={control_mode}: expected 0..{self.controlnet.num_mode - 1}")
            if not self.controlnet.is_union and control_mode is not None:
                raise ValueError("fluxmi: control_mode is for Union ControlNets; this net has no mode embedding")
            try:
                cg0, cg1 = float(control_guidance_start), float(control_guidance_end)
                cn_scale = float(controlnet_conditioning_scale)
            except (TypeError, ValueError):
                raise ValueError("fluxmi: controlnet_conditioning_scale / control_guidance_start / control_guidance_end: expected numbers") from None
            if not (0.0 <= cg0 <= 1.0 and 0.0 <= cg1 <= 1.0 and cg0 <= cg1 and math.isfinite(cn_scale)):
                raise ValueError(f"fluxmi: control_guidance_start={control_guidance_start} / end={control_guidance_end}: expected 0 <= start <= "
                                 f"end <= 1 and a finite controlnet_conditioning_scale")
            if fdist.world_size() > 1:
                raise ValueError("fluxmi: a ControlNet request under a process group is not supported")
        ip_on = ip_adapter_image is not None or ip_adapter_image_embeds is not None
        if ip_on:
            from modules.ip_adapter import scale_table

            if getattr(self, "ip_adapter", None) is None:
                raise ValueError("fluxmi: ip_adapter_image needs an IP-Adapter: set config.ip_adapter_path (a local XLabs-format "
                                 "flux-ip-adapter checkpoint) and config.clip_vision_path (the CLIP ViT-L/14 vision tower)")
            if ip_adapter_image is not None and ip_adapter_image_embeds is not None:
                raise ValueError("fluxmi: pass ip_adapter_image or ip_adapter_image_embeds, not both")
            if regions is not None:
                raise ValueError("fluxmi: regions do not combine with an IP-Adapter")
            if cache_on:
                raise ValueError("fluxmi: cache_threshold > 0 (step caching) does not combine with an IP-Adapter")
            if fdist.world_size() > 1:
                raise ValueError("fluxmi: an IP-Adapter request under a process group is not supported")
            depth = self.ip_adapter.depth
            if depth != len(self.model.double_blocks) or self.ip_adapter.hidden != self.model.hidden_size:
                raise ValueError(f"fluxmi: the IP-Adapter has {depth} double blocks of hidden {self.ip_adapter.hidden}, the flow model "
                                 f"{len(self.model.double_blocks)} of {self.model.hidden_size}")
            try:
                ip_scales = (scale_table(ip_adapter_scale, depth, 1), scale_table(negative_ip_adapter_scale, depth, 1))
            except (TypeError, ValueError) as e:
                raise ValueError(f"fluxmi: ip_adapter_scale / negative_ip_adapter_scale: {e}") from None
        elif negative_ip_adapter_image is not None:
            raise ValueError("fluxmi: negative_ip_adapter_image goes with ip_adapter_image / ip_adapter_image_embeds")
        if inpaint_mask is None and inpaint_differential:
            raise ValueError("fluxmi: inpaint_differential needs an inpaint_mask (the change map)")
        if inpaint_mask is not None and init_image is None:
            raise ValueError("fluxmi: inpaint_mask needs init_image (the image whose black-masked part is kept)")
        region_grids = None
        if regions is not None:
            if not isinstance(regions, (list, tuple)) or not regions:
                raise ValueError("fluxmi: regions must be a non-empty list of {'prompt', 'box' | 'mask'} entries")
            if not isinstance(regional_tokens, int) or regional_tokens < 16 or regional_tokens % 16:
                raise ValueError(f"fluxmi: regional_tokens={regional_tokens!r}: expected a positive multiple of 16")
            for r in regions:
                if not isinstance(r, dict) or "prompt" not in r:
                    raise ValueError("fluxmi: every region needs a 'prompt'")
            # a mask given as a path / base64 string is loaded like init_image
            regions = [{**r, "mask": self.load_init_image_if_needed(r["mask"])} if isinstance(r.get("mask"), str) else r for r in regions]
            region_grids = torch.stack([region_token_grid(r, 16 * (height // 16), 16 * (width // 16)) for r in regions])
            if len(regions) + 2 > ATTN_GROUPS:
                raise ValueError(f"fluxmi: {len(regions)} regions: at most {ATTN_GROUPS - 2} fit the {ATTN_GROUPS} attention groups")
        try:
            cache_threshold, cache_max_hits = float(cache_threshold), int(cache_max_hits)
        except (TypeError, ValueError):
            raise ValueError(f"fluxmi: cache_threshold={cache_threshold!r} / cache_max_hits={cache_max_hits!r}: expected a number and an integer") from None
        if not (math.isfinite(cache_threshold) and cache_threshold >= 0.0):
            raise ValueError(f"fluxmi: cache_threshold={cache_threshold}: expected a finite value >= 0 (0 = off)")
        if cache_max_hits < 0:
            raise ValueError(f"fluxmi: cache_max_hits={cache_max_hits}: expected >= 0 (0 = no bound)")
        cache = dict(cache_threshold=cache_threshold, cache_max_hits=cache_max_hits) if cache_threshold > 0 else {}
        if redux_image is not None:
            self._require_redux()
        if negative_prompt is None and true_cfg_scale > 1:
            raise ValueError(f"fluxmi: true_cfg_scale={true_cfg_scale} needs a negative_prompt (\"\" for the unconditional branch); without "
                             "one the request would pay for two branches and guide nothing")
        try:
            cfg_lo, cfg_hi = (float(v) for v in true_cfg_interval)
        except (TypeError, ValueError):
            raise ValueError(f"fluxmi: true_cfg_interval={true_cfg_interval!r}: expected (lo, hi)") from None
        if not 0.0 <= cfg_lo <= cfg_hi <= 1.0:
            raise ValueError(f"fluxmi: true_cfg_interval={true_cfg_interval!r}: expected 0 <= lo <= hi <= 1")
        guided = negative_prompt is not None and true_cfg_scale > 1
        kind = self.conditioning_kind()
        if kind is None and (mask_image is not None or control_image is not None or img_cond is not None):
            raise ValueError("fluxmi: mask_image / control_image / img_cond need a FLUX.1 Fill or Depth / Canny model (this one has no "
                             "conditioning channels)")
        if kind is not None:
            if reference_image is not None:
                raise ValueError("fluxmi: a Fill / Depth / Canny model takes no Kontext reference_image")
            if kind == "fill" and control_image is not None:
                raise ValueError("fluxmi: control_image is for FLUX.1 Depth / Canny; a Fill model takes init_image + mask_image")
            if kind == "control" and mask_image is not None:
                raise ValueError("fluxmi: mask_image is for FLUX.1 Fill; a Depth / Canny model takes control_image")
            if img_cond is not None and (mask_image is not None or control_image is not None):
                raise ValueError("fluxmi: pass img_cond or mask_image / control_image, not both")
            if img_cond is None and kind == "fill" and (mask_image is None or init_image is None):
                raise ValueError("fluxmi: FLUX.1 Fill needs init_image (the image to inpaint) and mask_image (white = regenerate)")
            if img_cond is None and kind == "control" and control_image is None:
                raise ValueError("fluxmi: FLUX.1 Depth / Canny needs control_image (the depth map or edge map)")
        num_steps = 4 if self.name == "flux-schnell" else num_steps
        if sigmas is not None:
            num_steps = len(sigmas) - 1
        init_image = self.load_init_image_if_needed(init_image) if init_image is not None else None
        fill_image = init_image if kind == "fill" else None
        if fill_image is not None and strength == 1.0 and inpaint_mask is None:
            init_image = None  # the img2img blend is the identity at strength 1: BFL's Fill starts from pure noise, no encode
        height, width = 16 * (height // 16), 16 * (width // 16)
        generator, seed = self.set_seed(seed)
        world, rank = fdist.world_size(), fdist.rank()
        cal = getattr(self.model, "calibration_state", None)
        # the batch prepare() will build: a list prompt with one noise sample sizes the batch by its length (flux_pipeline.py:267-278)
        eff_images = len(prompt) if (isinstance(prompt, (list, tuple)) and num_images == 1) else num_images
        if world > 1 and eff_images < world and cal is not None and cal()[0] is False:
            # every rank sees the same (batch, world, calibration state), so every rank raises -- before any collective.  A rank
            # with an empty shard would skip the calibrating steps: its trial counters would not advance and (with or without the in-step
            # amax exchange) the replicas would freeze different input scales, silently.
            raise RuntimeError(f"fluxmi: calibrating with fewer images ({eff_images}) than ranks ({world}); use num_images >= world_size "
                               "until the F8Linear input scales are frozen (FluxPipeline.compile() does)")
        # batch-sharded replicas: every rank denoises its own slice of the batch (rank 0's noise / init latent is
        # what the broadcast below distributes)
        inp_mask = self.prepare_inpaint_mask(inpaint_mask, height, width, bool(inpaint_differential)) if inpaint_mask is not None else None
        if inp_mask is None:
            noise, timesteps = self.preprocess_latent(init_image=init_image, height=height, width=width, num_steps=num_steps, strength=strength,
                                                      generator=generator, num_images=num_images, noise=noise, **sched_kw)
        else:
            noise, timesteps, inp_x0, inp_noise = self.preprocess_latent_parts(init_image=init_image, height=height, width=width, num_steps=num_steps,
                                                                               strength=strength, generator=generator, num_images=num_images, noise=noise, **sched_kw)
        img, img_ids, vec, txt, txt_ids = map(lambda x: x.contiguous(), self.prepare(noise, prompt))
        num_images = img.shape[0]  # a list prompt with num_images == 1 sizes the batch (prepare)
        inpaint = None
        if inp_mask is not None:
            # [x0 | noise | mask] per token, in the flow dtype (the mask's 0 / 1 / block means are what the engine's bf16 copy holds too)
            rep = lambda t: t.repeat_interleave(num_images // t.shape[0], dim=0) if t.shape[0] != num_images else t
            inpaint = torch.cat((rep(self.pack(inp_x0)), rep(self.pack(inp_noise)), inp_mask.to(img.dtype).expand(num_images, -1, -1)), -1).contiguous()
        neg_txt = neg_vec = None
        if guided:
            neg_vec, neg_txt = self._prepare_negative(negative_prompt, noise, num_images, txt)
        if redux_image is not None:
            if world > 1 and rank != 0:
                # the broadcast below carries rank 0's tokens; this rank only needs the same text length
                n_tok = len(self._redux_list(redux_image)) * self.redux.num_tokens
                txt = torch.cat((txt, txt.new_zeros(txt.shape[0], n_tok, txt.shape[2])), dim=-2)
                txt_ids = txt_ids.new_zeros(txt.shape[0], txt.shape[1], 3)
            else:
                txt, txt_ids = self.prepare_redux_tokens(redux_image, num_images=num_images, txt=txt)
            txt, txt_ids = txt.contiguous(), txt_ids.contiguous()
            if guided:  # the same image tokens behind the negative prompt's T5 tokens
                neg_txt = torch.cat((neg_txt, txt[:, neg_txt.shape[1]:]), dim=-2).contiguous()
        n_base = txt.shape[1]
        if regions is not None:
            rows = []
            for r in regions:
                r_txt = self._region_text(r["prompt"])
                if r_txt.shape[0] != 1 or r_txt.shape[1] < regional_tokens or r_txt.shape[2] != txt.shape[2]:
                    raise ValueError(f"fluxmi: a region prompt's T5 states {tuple(r_txt.shape)} hold fewer than regional_tokens={regional_tokens} rows")
                rows.append(r_txt[:, :regional_tokens].to(txt))
            rows = torch.cat(rows, 1).expand(txt.shape[0], -1, -1)
            txt = torch.cat((txt, rows), 1).contiguous()
            txt_ids = txt_ids.new_zeros(txt.shape[0], txt.shape[1], 3)
            if guided:  # the same rows in the negative branch, where the table hides them from every other token
                neg_txt = torch.cat((neg_txt, rows), 1).contiguous()
        cond = {}
        if reference_image is not None:
            # drawn from the request's generator after the noise (the order is part of what a seed reproduces)
            c_seq, c_ids = self.prepare_kontext_reference(reference_image, num_images=num_images, generator=generator)
            cond = dict(img_cond_seq=c_seq, img_cond_seq_ids=c_ids)
        if kind is not None:
            # drawn from the request's generator after the noise, like a Kontext reference
            if img_cond is None and kind == "fill":
                img_cond = self.prepare_fill_conditioning(fill_image, mask_image, height, width, num_images=1, generator=generator)
            elif img_cond is None:
                if control_preprocess is not None:
                    control_image = self.preprocess_control(control_image, control_preprocess, width, height, **prep_kw)
                img_cond = self.prepare_control_conditioning(control_image, height, width, num_images=1, generator=generator)
            img_cond = img_cond.to(device=self.device_flux, dtype=torch.bfloat16)
            if img_cond.shape[0] == 1 and num_images > 1:
                img_cond = img_cond.repeat(num_images, 1, 1)
            cond = dict(img_cond=img_cond.contiguous())
        cn_cond = None
        if cn_on:
            # drawn from the request's generator after the noise, like a Kontext reference
            if controlnet_cond is None:
                if control_preprocess is not None:
                    controlnet_image = self.preprocess_control(controlnet_image, control_preprocess, width, height, **prep_kw)
                controlnet_cond = self.prepare_controlnet_conditioning(controlnet_image, height, width, num_images=1, generator=generator)
            cn_cond = controlnet_cond.to(device=self.device_flux, dtype=torch.bfloat16)
            if cn_cond.ndim != 3 or cn_cond.shape[0] not in (1, num_images) or tuple(cn_cond.shape[1:]) != tuple(img.shape[1:]):
                raise ValueError(f"fluxmi: controlnet_cond {tuple(cn_cond.shape)}: expected [1 or {num_images}, {img.shape[1]}, {img.shape[2]}]")
            cn_cond = cn_cond.expand(num_images, -1, -1).contiguous()
        ip_calls = None
        if ip_on:
            ip_calls = self.prepare_ip_adapter(ip_adapter_image, ip_adapter_image_embeds, ip_scales[0],
                                               negative_ip_adapter_image if guided else None, ip_scales[1], guided)
        first_image = 0  # the request's index of this rank's first image (the noise ids of a stochastic sampler count from it)
        if world > 1:
            if guided:  # the negative embeddings ride in the one broadcast, behind the prompt's
                txt, vec = torch.cat((txt, neg_txt), 0), torch.cat((vec, neg_vec), 0)
            inp_kw = {} if inpaint is None else dict(inpaint=inpaint)  # rank 0's [x0 | noise | mask] rides in the same broadcast
            if "img_cond" in cond:
                # every rank steps rank 0's conditioning (the VAE sample differs between ranks' generators); its bf16 bits ride in the
                # payload's dtype and come back unchanged
                txt, vec, img, c, *got = fdist.broadcast_request(txt, vec, img, src=0, extra=cond["img_cond"].view(img.dtype), **inp_kw)
                cond["img_cond"] = c.view(torch.bfloat16)
            elif cond:
                # every rank steps rank 0's reference latents (the VAE sample differs between ranks' generators on other devices)
                txt, vec, img, cond["img_cond_seq"], *got = fdist.broadcast_request(txt, vec, img, src=0, extra=cond["img_cond_seq"], **inp_kw)
            else:
                txt, vec, img, *got = fdist.broadcast_request(txt, vec, img, src=0, **inp_kw)
            if inpaint is not None:
                inpaint = got[0]
            if guided:
                (txt, neg_txt), (vec, neg_vec) = txt.chunk(2, 0), vec.chunk(2, 0)
            # images are sharded, not branches: both branches of an image run on the rank that owns it
            lo, hi = fdist.shard_bounds(img.shape[0], rank, world)
            first_image = lo
            img, img_ids, vec, txt, txt_ids = (t[lo:hi].contiguous() for t in (img, img_ids, vec, txt, txt_ids))
            if guided:
                neg_txt, neg_vec = neg_txt[lo:hi].contiguous(), neg_vec[lo:hi].contiguous()
            cond = {k: v[lo:hi].contiguous() for k, v in cond.items()}
            if inpaint is not None:
                inpaint = inpaint[lo:hi].contiguous()
        if img.shape[0] == 0:
            # more ranks than images (frozen scales only, see above): this rank has nothing to denoise but still takes part in the gather
            # below (an exception or an early return here would leave the other ranks blocked in the collective)
            latents = img.new_empty((0,) + tuple(img.shape[1:]))
        else:
            n = len(timesteps) - 1
            # step i is guided iff cfg_lo n <= i < cfg_hi n, i.e. ceil(cfg_lo n) <= i < ceil(cfg_hi n)
            g0, g1 = (min(n, math.ceil(cfg_lo * n)), min(n, math.ceil(cfg_hi * n))) if guided else (n, n)
            neg = dict(neg_txt=neg_txt, neg_y=neg_vec, cfg_scale=true_cfg_scale)
            plain_kw = {}
            if regions is not None:
                n_ref = cond["img_cond_seq"].shape[1] if "img_cond_seq" in cond else 0
                tab = [build_region_groups(n_base, regional_tokens, region_grids, n_ref=n_ref, negative=ng) for ng in ((False, True) if guided else (False,))]
                plain_kw = dict(attn_groups=tab[0][None].to(self.device_flux))
                neg["attn_groups"] = torch.stack(tab).to(self.device_flux)
            if ip_calls is not None:  # the prompt branch's tables for the unguided steps, both branches' for the guided ones
                plain_kw = dict(plain_kw, ip_adapter=ip_calls[0])
                neg["ip_adapter"] = ip_calls[1]
            thr = self.inpaint_thresholds(n) if inpaint is not None and inpaint_differential else None
            latents = img
            if stochastic:  # per-image ids of the noise: the request's image index, not the rank's or the pass's
                key = int(seed if noise_seed is None else noise_seed)
                noise_ids = [(key & 0xffffffff, (key >> 32) & 0xffffffff, first_image + k, 0) for k in range(img.shape[0])]
            segs = list(((0, g0, plain_kw), (g0, g1, neg), (g1, n, plain_kw)) if g0 < g1 else ((0, n, plain_kw),))
            if cn_cond is not None and n > 0:
                # cut every segment where the ControlNet switches on or off (diffusers' controlnet_keep): consecutive denoise calls
                from modules.controlnet import ControlNetCall, control_steps

                keep = control_steps(n, cg0, cg1)
                call = ControlNetCall(self.controlnet, cn_cond, cn_scale, None if control_mode is None else int(control_mode))
                cut = []
                for a, b, kw in segs:
                    i = a
                    while i < b:
                        j = i
                        while j < b and keep[j] == keep[i]:
                            j += 1
                        cut.append((i, j, dict(kw, controlnet=call) if keep[i] else kw))
                        i = j
                segs = cut
            evals_done = 0  # model evaluations of the request in front of the segment (zero_init_steps counts them)
            plan = []  # the denoise calls of the request: (a, b, keywords), every keyword but those that count evaluations
            for a, b, kw in segs:
                if a < b or n == 0:
                    if shaping is not None and "neg_txt" in kw:
                        kw = dict(kw, guidance_shaping=dict(shaping, step_offset=evals_done))
                    if inpaint is not None:
                        x0_, noise_, mask_ = inpaint.chunk(3, -1)
                        kw = dict(kw, inpaint_x0=x0_, inpaint_noise=noise_, inpaint_mask=mask_)
                        if thr is not None:
                            kw["inpaint_thresholds"] = thr[a:b]  # each denoise call gets its slice of the request's table
                    if stochastic:  # ... one evaluation per step: the slice's first evaluation is the request's a-th
                        kw = dict(kw, solver=solvers.build_program(sampler, timesteps[a:b + 1], eta, s_noise))
                        if solvers.has_noise(kw["solver"]):  # eta = 0, s_noise = 0 or a slice that is only the step onto 0 draws nothing
                            kw["solver_noise"] = (noise_ids, a)
                    elif sampler != "euler":  # ... and the program of its slice of the schedule
                        kw = dict(kw, solver=solvers.build_program(sampler, timesteps[a:b + 1]))
                    plan.append((a, b, kw, evals_done))
                    evals_done += len(kw["solver"].coef) if "solver" in kw else b - a
            for a, b, kw, off in plan:
                if on_step is not None:  # the request's numbering continues across its denoise calls
                    kw = dict(kw, preview=self._preview_call(on_step, preview_proj, preview_every, height, width, a, off, evals_done, kw.get("solver")))
                latents = self.model.denoise(latents, img_ids, txt, txt_ids, vec, timesteps[a:b + 1], guidance=guidance, use_graph=use_graph,
                                             **cond, **kw, **cache)
        if world > 1:
            latents = fdist.gather_latents(latents, num_images, dst=0)
            if latents is None:  # only the gather rank decodes / returns the images
                return (None, seed) if return_seed else None
        if output_type == "latent" or self.ae is None:
            out = self.unpack(latents.float(), height, width) if latents is not None else None
            return (out, seed) if return_seed else out
        img_px = self.vae_decode(latents, height, width)
        # output_type "uint8": the [B, H, W, 3] array into_bytes hands to the JPEG encoder (the pixel-parity tests compare it)
        out = self._pixels_out(img_px, output_type, jpeg_quality, upscale, jpeg_encoder)
        return (out, seed) if return_seed else out

    # ---- tiled generation (fluxmi.windows; Flux.denoise_windows) -------------------------------------------------------------------------------
    VAE_MAX_LATENT_PIXELS = 46340  # the VAE's mid-block attention scores [P, P] bf16 behind a 32-bit GEMM descriptor: 2 P^2 bytes < 4 GiB
    # vae_attention="streaming" has no score matrix.  What is left behind a 32-bit descriptor is the A operand of the 1x1-convolution GEMMs:
    # the widest at full resolution is 64 P pixels x 256 channels x 2 bytes < 4 GiB, i.e. P < 131072 per image (DESIGN.md section 7;
    # AutoEncoder decodes / encodes batches above that image by image)
    VAE_MAX_LATENT_PIXELS_STREAMING = 131071
    vae_attention = "gemm"  # the config's ModelSpec.vae_attention, carried to self.ae.attention by the constructor

    def _check_tiles(self, a: dict):
        """generate's arguments -> None (no tile_size, or one tile of the request's size and nothing else asked: today's request) or the
        fluxmi.windows.WindowPlan of the request; every refusal of a tiled request is raised here, before any encoder or engine work"""
        from fluxmi import windows
        from modules.flux_model import Flux

        ts, ov, prof = a["tile_size"], a["tile_overlap"], a["tile_weight"]
        if ts is None:
            if ov is not None or prof != "cosine":
                raise ValueError("fluxmi: tile_overlap / tile_weight belong to a tiled request: they need tile_size")
            return None
        is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)
        if is_int(ts):
            ts = (ts, ts)
        if not isinstance(ts, (tuple, list)) or len(ts) != 2 or not all(is_int(v) for v in ts):
            raise ValueError(f"fluxmi: tile_size={a['tile_size']!r}: expected an int or (height, width) in pixels")
        th, tw = ts
        height, width = 16 * (a["height"] // 16), 16 * (a["width"] // 16)
        if th < 16 or tw < 16 or th % 16 or tw % 16 or th > height or tw > width:
            raise ValueError(f"fluxmi: tile_size={a['tile_size']!r}: expected multiples of 16, at least 16 and at most the request's {height} x "
                             f"{width} (height x width)")
        if prof not in windows.PROFILES:
            raise ValueError(f"fluxmi: tile_weight={prof!r}: expected one of {windows.PROFILES}")
        if ov is not None and (not is_int(ov) or ov < 0 or ov % 16 or ov >= min(th, tw)):
            raise ValueError(f"fluxmi: tile_overlap={ov!r}: expected a multiple of 16 with 0 <= overlap < tile ({min(th, tw)})")
        if (th, tw) == (height, width) and ov is None and prof == "cosine":
            return None
        no = lambda what: ValueError(f"fluxmi: tile_size (tiled generation) does not combine with {what}")
        if a["sampler"] != "euler" or a["eta"] != 1.0 or a["s_noise"] != 1.0 or a["noise_seed"] is not None:
            raise no(f"sampler={a['sampler']!r} / eta / s_noise / noise_seed (the windowed update is an Euler step: sampler \"euler\" only)")
        if (a["guidance_mode"] != "cfg" or a["guidance_rescale"] != 0.0 or a["zero_init_steps"] != 0 or a["apg_eta"] != 1.0
                or a["apg_norm_threshold"] != 0.0 or a["apg_momentum"] != 0.0):
            raise no("guidance shaping (guidance_mode / guidance_rescale / apg_* / zero_init_steps: a guided tiled request is unshaped)")
        for name, what in (("inpaint_mask", "inpaint_mask"), ("reference_image", "a Kontext reference_image"), ("redux_image", "redux_image"),
                           ("regions", "regions"), ("source_prompt", "source_prompt (FlowEdit)"), ("mask_image", "mask_image (FLUX.1 Fill)"),
                           ("control_image", "control_image (FLUX.1 Depth / Canny)"), ("img_cond", "img_cond (FLUX.1 Fill / Depth / Canny)")):
            if a[name] is not None:
                raise no(what)
        if a["inpaint_differential"]:
            raise no("inpaint_differential")
        if a["controlnet_image"] is not None or a["controlnet_cond"] is not None:
            raise no("a ControlNet")
        if a["ip_adapter_image"] is not None or a["ip_adapter_image_embeds"] is not None or a["negative_ip_adapter_image"] is not None:
            raise no("an IP-Adapter")
        try:
            cache_on = float(a["cache_threshold"]) > 0
        except (TypeError, ValueError):
            cache_on = True
        if cache_on:
            raise no("cache_threshold > 0 (step caching)")
        pe = a["preview_every"]
        if isinstance(pe, bool) or not isinstance(pe, int) or pe != 0 or a["preview_factors"] is not None:
            raise no("preview_every > 0 (the stream holds windows, not the canvas; on_step reports progress and cancels)")
        if a["on_step"] is not None and not callable(a["on_step"]):
            raise ValueError("fluxmi: on_step must be callable")
        if fdist.world_size() > 1:
            raise no("a process group")
        if self.conditioning_kind() is not None:
            raise no("a FLUX.1 Fill / Depth / Canny model")
        if a["sigma_schedule"] not in solvers.SIGMA_SCHEDULES:
            raise ValueError(f"fluxmi: sigma_schedule={a['sigma_schedule']!r}: expected one of {solvers.SIGMA_SCHEDULES}")
        if a["negative_prompt"] is None and a["true_cfg_scale"] > 1:
            raise ValueError(f"fluxmi: true_cfg_scale={a['true_cfg_scale']} needs a negative_prompt")
        try:
            lo, hi = (float(v) for v in a["true_cfg_interval"])
        except (TypeError, ValueError):
            raise ValueError(f"fluxmi: true_cfg_interval={a['true_cfg_interval']!r}: expected (lo, hi)") from None
        if not 0.0 <= lo <= hi <= 1.0:
            raise ValueError(f"fluxmi: true_cfg_interval={a['true_cfg_interval']!r}: expected 0 <= lo <= hi <= 1")
        ovh, ovw = (16 * (th // 64), 16 * (tw // 64)) if ov is None else (ov, ov)
        plan = windows.plan(height // 16, width // 16, th // 16, tw // 16, (th - ovh) // 16, (tw - ovw) // 16, prof)
        n_img = a["num_images"]
        if isinstance(n_img, bool) or not isinstance(n_img, int) or n_img < 1:
            raise ValueError(f"fluxmi: num_images={n_img!r}: expected an integer >= 1")
        if isinstance(a["prompt"], (list, tuple)) and n_img == 1:
            n_img = max(1, len(a["prompt"]))
        guided = a["negative_prompt"] is not None and a["true_cfg_scale"] > 1
        cap = Flux.MAX_ENGINE_BATCH // 2 if guided else Flux.MAX_ENGINE_BATCH
        if n_img * plan.ny * plan.nx > cap:
            raise no(f"num_images={n_img} at this size: {n_img} x {plan.ny} x {plan.nx} windows do not fit one engine pass of {cap} samples"
                     f"{' (half the pass: a negative prompt doubles them)' if guided else ''}; use a larger tile_size or a smaller tile_overlap")
        decodes = not (a["output_type"] == "latent" or self.ae is None)
        if check_attention_mode(self.vae_attention) == "streaming":
            if (decodes or a["init_image"] is not None) and (height // 8) * (width // 8) > self.VAE_MAX_LATENT_PIXELS_STREAMING:
                raise no(f"{'init_image' if a['init_image'] is not None else 'a decoded output'} at {height} x {width}: the VAE's full-resolution "
                         f"activations of the canvas's P = {(height // 8) * (width // 8)} latent pixels sit behind 32-bit GEMM descriptors "
                         f"(P <= {self.VAE_MAX_LATENT_PIXELS_STREAMING} with vae_attention=\"streaming\"); a text-to-image request can return "
                         f"output_type=\"latent\"")
        elif (decodes or a["init_image"] is not None) and (height // 8) * (width // 8) > self.VAE_MAX_LATENT_PIXELS:
            raise no(f"{'init_image' if a['init_image'] is not None else 'a decoded output'} at {height} x {width}: the VAE's mid-block attention "
                     f"holds a [P, P] bf16 score matrix of the canvas's P = {(height // 8) * (width // 8)} latent pixels behind a 32-bit GEMM "
                     f"descriptor (P <= {self.VAE_MAX_LATENT_PIXELS}); the config's vae_attention=\"streaming\" has no such matrix, and a "
                     f"text-to-image request can return output_type=\"latent\"")
        return plan

    def _generate_tiled(self, plan, prompt, width, height, num_steps, guidance, seed, init_image, strength, num_images, return_seed, jpeg_quality,
                        output_type, noise, use_graph, negative_prompt, true_cfg_scale, true_cfg_interval, sigma_schedule, sigmas, on_step,
                        upscale=False, jpeg_encoder="pil"):
        """the tiled request of generate (its docstring): today's noise / img2img / text at canvas size, then Flux.denoise_windows on the
        canvas -- one call, or up to three where true_cfg_interval cuts the request"""
        from modules.flux_model import Flux, PreviewCall

        num_steps = 4 if self.name == "flux-schnell" else num_steps
        if sigmas is not None:
            sigmas = solvers.custom_sigmas(sigmas)
            num_steps = len(sigmas) - 1
        sched_kw = {k: v for k, v in (("sigmas", sigmas), ("sigma_schedule", sigma_schedule)) if v is not None}
        init_image = self.load_init_image_if_needed(init_image) if init_image is not None else None
        height, width = 16 * (height // 16), 16 * (width // 16)
        generator, seed = self.set_seed(seed)
        # the schedule's shift follows the WINDOW's sequence length: that is the image the model sees
        x, timesteps = self.preprocess_latent(init_image=init_image, height=height, width=width, num_steps=num_steps, strength=strength,
                                              generator=generator, num_images=num_images, noise=noise, image_seq_len=plan.h * plan.w, **sched_kw)
        img, _, vec, txt, txt_ids = map(lambda t: t.contiguous(), self.prepare(x, prompt))
        N = img.shape[0]  # a list prompt with num_images == 1 sizes the batch (prepare)
        guided = negative_prompt is not None and true_cfg_scale > 1
        cap = Flux.MAX_ENGINE_BATCH // 2 if guided else Flux.MAX_ENGINE_BATCH
        if N * plan.ny * plan.nx > cap:
            raise ValueError(f"fluxmi: tile_size (tiled generation): {N} images x {plan.ny} x {plan.nx} windows do not fit one engine pass of {cap} samples")
        neg = {}
        if guided:
            neg_vec, neg_txt = self._prepare_negative(negative_prompt, x, N, txt)
            neg = dict(neg_txt=neg_txt, neg_y=neg_vec, cfg_scale=true_cfg_scale)
        win_ids = self.make_img_ids(1, plan.h, plan.w, self.device_flux, self.dtype)
        canvas = img.reshape(N, plan.Hc, plan.Wc, img.shape[2])  # pack() is row-major over the token grid
        n = len(timesteps) - 1
        cfg_lo, cfg_hi = (float(v) for v in true_cfg_interval)
        g0, g1 = (min(n, math.ceil(cfg_lo * n)), min(n, math.ceil(cfg_hi * n))) if guided else (n, n)
        segs = list(((0, g0, {}), (g0, g1, neg), (g1, n, {})) if g0 < g1 else ((0, n, {}),))
        for a, b, kw in segs:
            if a < b or n == 0:
                if on_step is not None:  # the request's numbering continues across its denoise calls
                    cb = lambda evaluation, num_evaluations, rgb, a=a: on_step({"evaluation": evaluation, "num_evaluations": num_evaluations,
                                                                                "step": evaluation, "preview": None})
                    kw = dict(kw, preview=PreviewCall(None, (0, 0), 0, a, n, cb))
                canvas = self.model.denoise_windows(canvas, plan, win_ids, txt, txt_ids, vec, timesteps[a:b + 1], guidance=guidance,
                                                    use_graph=use_graph, **kw)
        latents = canvas.reshape(N, plan.Hc * plan.Wc, -1).to(img.dtype)
        if output_type == "latent" or self.ae is None:
            out = self.unpack(latents.float(), height, width)
            return (out, seed) if return_seed else out
        img_px = self.vae_decode(latents, height, width)
        out = self._pixels_out(img_px, output_type, jpeg_quality, upscale, jpeg_encoder)
        return (out, seed) if return_seed else out

    # ---- FlowEdit (fluxmi.flowedit; Flux.denoise_edit) ---------------------------------------------------------------------------------------
    def _check_edit(self, a: dict):
        """generate's arguments -> None (no source_prompt: today's request) or (source_guidance, n_max, n_min, n_avg); every refusal of an
        edit request is raised here, before any encoder or engine work"""
        from fluxmi import flowedit

        if a["source_prompt"] is None:
            if a["source_guidance"] is not None or a["edit_n_max"] is not None or a["edit_n_min"] != 0 or a["edit_n_avg"] != 1:
                raise ValueError("fluxmi: source_guidance / edit_n_max / edit_n_min / edit_n_avg belong to a FlowEdit request: they need source_prompt")
            return None
        no = lambda what: ValueError(f"fluxmi: source_prompt (FlowEdit) does not combine with {what}")
        if a["init_image"] is None:
            raise ValueError("fluxmi: source_prompt (FlowEdit) needs init_image (the image the source prompt describes)")
        if a["strength"] != 1.0:
            raise ValueError(f"fluxmi: source_prompt (FlowEdit) needs strength 1.0, not {a['strength']} (edit_n_max bounds how far the edit goes)")
        if a["sampler"] != "euler" or a["eta"] != 1.0 or a["s_noise"] != 1.0:
            raise ValueError(f"fluxmi: source_prompt (FlowEdit) needs sampler \"euler\" (got {a['sampler']!r}) and takes no eta / s_noise")
        if a["negative_prompt"] is not None and a["true_cfg_scale"] > 1:
            raise no("a negative_prompt at true_cfg_scale > 1 (four branches per image)")
        for name in ("inpaint_mask", "reference_image", "regions", "redux_image", "mask_image", "control_image", "img_cond"):
            if a[name] is not None:
                raise no(name)
        if a["controlnet_image"] is not None or a["controlnet_cond"] is not None:
            raise no("a ControlNet")
        if a["ip_adapter_image"] is not None or a["ip_adapter_image_embeds"] is not None:
            raise no("an IP-Adapter")
        try:
            cache_on = float(a["cache_threshold"]) > 0
        except (TypeError, ValueError):
            cache_on = True
        if cache_on:
            raise no("cache_threshold > 0 (every evaluation runs on a fresh draw)")
        pe = a["preview_every"]
        if isinstance(pe, bool) or not isinstance(pe, int) or pe != 0:
            raise no("preview_every > 0 (there are no previews of the edit state; on_step reports progress and cancels)")
        if a["on_step"] is not None and not callable(a["on_step"]):
            raise ValueError("fluxmi: on_step must be callable")
        if fdist.world_size() > 1:
            raise no("a process group")
        if self.conditioning_kind() is not None:
            raise no("a FLUX.1 Fill / Depth / Canny model")
        sg = a["guidance"] if a["source_guidance"] is None else a["source_guidance"]
        try:
            sg = float(sg)
            if not math.isfinite(sg):
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError(f"fluxmi: source_guidance={a['source_guidance']!r}: expected a finite number") from None
        ns = a["noise_seed"]
        if ns is not None and (isinstance(ns, bool) or not isinstance(ns, int) or not 0 <= ns < 2 ** 64):
            raise ValueError(f"fluxmi: noise_seed={ns!r}: expected an integer in [0, 2^64)")
        if a["sigma_schedule"] not in solvers.SIGMA_SCHEDULES:
            raise ValueError(f"fluxmi: sigma_schedule={a['sigma_schedule']!r}: expected one of {solvers.SIGMA_SCHEDULES}")
        if isinstance(a["num_images"], bool) or not 1 <= a["num_images"] <= flowedit.MAX_IMAGES:
            raise ValueError(f"fluxmi: source_prompt (FlowEdit) takes 1..{flowedit.MAX_IMAGES} images per request, not {a['num_images']}")
        steps = 4 if self.name == "flux-schnell" else a["num_steps"]
        if a["sigmas"] is not None:
            steps = len(solvers.custom_sigmas(a["sigmas"])) - 1
        flowedit.build_program((1.0, 0.0), a["edit_n_avg"])  # edit_n_avg < 1: refused here
        flowedit.split_steps(steps, a["edit_n_max"], a["edit_n_min"])  # 0 <= edit_n_min <= edit_n_max <= num_steps, or refused
        return sg, a["edit_n_max"], a["edit_n_min"], a["edit_n_avg"]

    @torch.inference_mode()
    def prepare_edit(self, init_image, height: int, width: int, num_steps: int, num_images: int = 1, sigmas=None, sigma_schedule=None):
        """-> (the VAE latent of `init_image` [num_images, 16, height / 8, width / 8] in the flow dtype, the request's schedule): what
        preprocess_latent_parts does with an init image at strength 1, without any draw: no noise (FlowEdit draws nothing from the
        generator) and the encoder's mean instead of a sample of its Gaussian"""
        if self.ae is None:
            raise RuntimeError("fluxmi: FlowEdit needs an autoencoder (config.ae_path) -- none is attached")
        if isinstance(init_image, np.ndarray):
            init_image = torch.from_numpy(init_image)
        px = init_image.permute(2, 0, 1).contiguous().to(self.device_ae, dtype=self.ae_dtype).div(127.5).sub(1)[None, ...]
        px = self.resize_center_crop(px, height, width)
        # x0 is the MEAN of the encoder's Gaussian (its mode, as the FlowEdit authors take it), not a sample: the edit starts from the photo
        # itself, and the same request gives the same bits without a draw
        mean = torch.chunk(self.ae.encode_moments(px), 2, dim=self.ae.reg.chunk_dim)[0].float()
        latent = (self.ae.scale_factor * (mean - self.ae.shift_factor)).to(dtype=self.dtype, device=self.device_flux).repeat(num_images, 1, 1, 1)
        timesteps = self.get_schedule(num_steps, latent.shape[-1] * latent.shape[-2] // 4, shift=(self.name != "flux-schnell"))
        if sigmas is not None:
            timesteps = [float(v) for v in sigmas]
        if sigma_schedule is not None:
            timesteps = solvers.sigma_schedule(sigma_schedule, timesteps)
        return latent, timesteps

    def _generate_edit(self, edit, prompt, source_prompt, width, height, num_steps, guidance, seed, init_image, silent, num_images, return_seed,
                       jpeg_quality, output_type, use_graph, sigma_schedule, sigmas, noise_seed, on_step, upscale=False,
                       jpeg_encoder="pil"):
        """the FlowEdit request of generate (its docstring): skipped steps | coupled steps (Flux.denoise_edit) | Euler tail (Flux.denoise)"""
        from fluxmi import flowedit, ops
        from modules.flux_model import PreviewCall

        source_guidance, n_max, n_min, n_avg = edit
        num_steps = 4 if self.name == "flux-schnell" else num_steps
        if sigmas is not None:
            sigmas = solvers.custom_sigmas(sigmas)
            num_steps = len(sigmas) - 1
        height, width = 16 * (height // 16), 16 * (width // 16)
        _, seed = self.set_seed(seed)
        init_image = self.load_init_image_if_needed(init_image)
        latent, timesteps = self.prepare_edit(init_image, height, width, num_steps, num_images, sigmas, sigma_schedule)
        x0, img_ids, vec, txt, txt_ids = map(lambda t: t.contiguous(), self.prepare(latent, prompt))
        _, _, src_vec, src_txt, _ = self.prepare(latent, source_prompt)
        if tuple(src_txt.shape[1:]) != tuple(txt.shape[1:]) or src_txt.shape[0] not in (1, txt.shape[0]):
            raise ValueError(f"fluxmi: source_prompt embeddings {tuple(src_txt.shape)} do not match the prompt's {tuple(txt.shape)}: both branches "
                             f"run in one batch, so they need the same sequence length")
        B = x0.shape[0]
        if B > flowedit.MAX_IMAGES:
            raise ValueError(f"fluxmi: source_prompt (FlowEdit) takes 1..{flowedit.MAX_IMAGES} images per request, not {B}")
        a, b = flowedit.split_steps(len(timesteps) - 1, n_max, n_min)
        ids = flowedit.edit_ids(seed if noise_seed is None else noise_seed, B)
        n_coupled, n_total = (b - a) * n_avg, (b - a) * n_avg + (len(timesteps) - 1 - b)

        def hook(eval_offset, step_of):  # the request's numbering continues from the coupled steps into the tail
            if on_step is None:
                return None
            cb = lambda evaluation, num_evaluations, rgb: on_step({"evaluation": evaluation, "num_evaluations": num_evaluations,
                                                                   "step": step_of(evaluation - eval_offset), "preview": None})
            return PreviewCall(None, (0, 0), 0, eval_offset, n_total, cb)

        z = x0
        if b > a:
            z = self.model.denoise_edit(x0, img_ids, src_txt, src_vec, txt, vec, txt_ids, timesteps[a:b + 1], n_avg=n_avg, ids=ids, eval_offset=0,
                                        source_guidance=source_guidance, guidance=guidance, use_graph=use_graph,
                                        preview=hook(0, lambda j: a + j // n_avg), x0=x0)
        latents = z
        if b < len(timesteps) - 1:
            # the tail: one coupling at the tail's first time with the next draw index -- n_coupled, the index a continuing edit call would
            # start at -- whose target half is an ordinary noisy latent of the edited image
            zt = ops.flowedit_couple(z.to(torch.bfloat16).contiguous(), x0.to(torch.bfloat16).contiguous(), timesteps[b], ids, n_coupled)[B:]
            latents = self.model.denoise(zt.to(x0.dtype), img_ids, txt, txt_ids, vec, timesteps[b:], guidance=guidance, use_graph=use_graph,
                                         **({} if on_step is None else dict(preview=hook(n_coupled, lambda j: b + j))))
        if output_type == "latent" or self.ae is None:
            out = self.unpack(latents.float(), height, width)
            return (out, seed) if return_seed else out
        img_px = self.vae_decode(latents, height, width)
        out = self._pixels_out(img_px, output_type, jpeg_quality, upscale, jpeg_encoder)
        return (out, seed) if return_seed else out

    def _preview_call(self, on_step, proj, every: int, height: int, width: int, step0: int, eval_offset: int, n_evaluations: int, solver):
        """the PreviewCall of one denoise call of a request: evaluation numbers are the request's, `step` goes through the slice's solver"""
        from modules.flux_model import PreviewCall

        def callback(evaluation, num_evaluations, rgb):
            j = evaluation - eval_offset
            step = step0 + (int(solver.step_of_eval[j]) if solver is not None else j)
            return on_step({"evaluation": evaluation, "num_evaluations": num_evaluations, "step": step, "preview": rgb})

        return PreviewCall(proj, (math.ceil(height / 16), math.ceil(width / 16)), every, eval_offset, n_evaluations, callback)

    def preview_projection(self, preview_factors=None) -> list:
        """The 51 floats the engine's preview launch reads, for the model's latent: `preview_factors` = (M [16][3], bias [3]) in
        decoded-latent space, else the config's, else the cached least-squares fit against this pipeline's VAE; the VAE's scale_factor /
        shift_factor are folded in (util.fold_preview_factors)."""
        from util import fit_preview_factors, fold_preview_factors

        ae = self.config.ae_params
        if preview_factors is None and getattr(self.config, "preview_factors", None) is not None:
            preview_factors = (self.config.preview_factors, self.config.preview_bias or [0.0, 0.0, 0.0])
        if preview_factors is None:
            if getattr(self, "_preview_fit", None) is None:
                if self.ae is None:
                    raise ValueError("fluxmi: preview_every > 0 needs preview_factors (or the config's) when no autoencoder is loaded")
                # a few seeded N(0, 1) latents through the native decoder, area-averaged 8 x 8 to latent resolution
                g = torch.Generator().manual_seed(0)
                z = torch.randn(4, ae.z_channels, 16, 16, generator=g).to(self.device_ae)
                with torch.autocast(device_type=self.device_ae.type, dtype=torch.bfloat16, cache_enabled=False):
                    px = self.ae.decode(z).float()
                f = px.shape[-1] // z.shape[-1]
                self._preview_fit = fit_preview_factors(z.float() / ae.scale_factor + ae.shift_factor, torch.nn.functional.avg_pool2d(px, f))
            preview_factors = self._preview_fit
        try:
            m, b = preview_factors
            return fold_preview_factors(m, b, ae.scale_factor, ae.shift_factor)
        except (TypeError, ValueError):
            raise ValueError("fluxmi: preview_factors: expected ([16][3], [3]): the matrix and the bias in decoded-latent space") from None

    def vae_decode(self, x: torch.Tensor, height: int, width: int) -> torch.Tensor:
        x = self.unpack(x.to(self.device_ae).float(), height, width)
        with torch.autocast(device_type=self.device_ae.type, dtype=torch.bfloat16, cache_enabled=False):
            return self.ae.decode(x)

    @staticmethod
    def to_uint8(x: torch.Tensor) -> torch.Tensor:
        """[B, 3, H, W] in [-1, 1] -> [B, H, W, 3] uint8 on the host (reference flux_pipeline.py:385-393)"""
        return x.clamp(-1, 1).add(1.0).mul(127.5).clamp(0, 255).permute(0, 2, 3, 1).contiguous().to(torch.uint8).cpu()

    @staticmethod
    def to_uint8_device(x: torch.Tensor) -> torch.Tensor:
        """to_uint8's arithmetic without the copy to the host: [B, 3, H, W] in [-1, 1] -> [B, H, W, 3] uint8 where x lives"""
        return x.clamp(-1, 1).add(1.0).mul(127.5).clamp(0, 255).permute(0, 2, 3, 1).contiguous().to(torch.uint8)

    def into_bytes(self, x: torch.Tensor, jpeg_quality: int = 99, jpeg_encoder: Optional[str] = None) -> io.BytesIO:
        if self._jpeg_encoder(jpeg_encoder) == "native":
            return self._jpeg_native(self.to_uint8_device(x), jpeg_quality)
        return self._jpeg(self.to_uint8(x), jpeg_quality)

    def _jpeg_encoder(self, jpeg_encoder: Optional[str]) -> str:
        """the request's encoder: its own `jpeg_encoder`, else the configuration's (ModelSpec.jpeg_encoder, "pil" when absent); an unknown
        value is refused by name"""
        enc = jpeg_encoder if jpeg_encoder is not None else getattr(getattr(self, "config", None), "jpeg_encoder", "pil")
        if enc not in JPEG_ENCODERS:
            raise ValueError(f"fluxmi: jpeg_encoder={enc!r}: expected one of {JPEG_ENCODERS}")
        return enc

    @staticmethod
    def _check_jpeg_native(num_images: int, height: int, width: int, jpeg_quality):
        """the native encoder's refusals, by name, before any other work of the request (fluxmi.ops.jpeg_params)"""
        from fluxmi import ops

        ops.jpeg_params(max(1, int(num_images)), height, width, jpeg_quality)

    @staticmethod
    def _jpeg_native(px: torch.Tensor, jpeg_quality: int = 99) -> io.BytesIO:
        """_jpeg on the device (fluxmi.ops.jpeg_encode): uint8 [B, H, W, 3] where the VAE left it -> the file, the batch stacked vertically;
        4:2:0 and the Annex K tables at `jpeg_quality`, which is what _jpeg's Pillow call picks, so both decode to the same pixels"""
        from fluxmi import ops

        with torch.cuda.device(px.device):  # the encoder launches on the current stream: make it the pixels' device's
            buf = io.BytesIO(ops.jpeg_encode(px, quality=jpeg_quality))
        buf.seek(0)
        return buf

    # ---- super-resolution (modules/upscaler.RRDBNet on fluxmi_conv3x3_dense) ---------------------------------------------------------------
    def _require_upscaler(self):
        if getattr(self, "upscaler", None) is None:
            raise ValueError("fluxmi: upscaling needs an ESRGAN-family checkpoint: set config.upscaler_path to a local RRDBNet .safetensors / "
                             ".pth file (nothing is downloaded)")
        return self.upscaler

    def upscale(self, image) -> torch.Tensor:
        """One image in any form `init_image` takes (path, base64 / data-URL, PIL image, HWC uint8 array or tensor), or a uint8 batch
        [B, H, W, 3] -> uint8 [B, scale H, scale W, 3] on the host through the configured RRDBNet: / 255 -> bf16 -> network -> clamp [0, 1]
        -> * 255, round half even.  An input the kernel's addressing or the free memory cannot take is refused by name; the network is
        not tiled."""
        net = self._require_upscaler()
        px = self.load_init_image_if_needed(image)
        if not isinstance(px, torch.Tensor) or px.dtype != torch.uint8:
            raise ValueError("fluxmi: upscale takes uint8 pixels (an image, or a [B, H, W, 3] uint8 batch)")
        if px.ndim == 2:
            px = px[..., None].expand(-1, -1, 3)
        if px.ndim == 3:
            px = px[None]
        if px.ndim != 4 or px.shape[-1] not in (3, 4):
            raise ValueError(f"fluxmi: upscale takes RGB pixels [H, W, 3] or [B, H, W, 3], got {tuple(px.shape)}")
        return net.upscale_uint8(px[..., :3].contiguous())

    def _check_upscale(self, upscale, init_upscale, output_type, init_image, width, height, num_images):
        """every refusal of generate's `upscale` / `init_upscale`, before any other work; -> init_image (upscaled when asked)"""
        net = self._require_upscaler()
        if upscale and (output_type == "latent" or self.ae is None):
            raise ValueError("fluxmi: upscale=True works on pixels: it cannot be combined with output_type=\"latent\" (or a pipeline without a VAE)")
        if init_upscale and init_image is None:
            raise ValueError("fluxmi: init_upscale=True needs init_image (the image to super-resolve before img2img)")
        if upscale:
            net.check_input(max(1, int(num_images)), 16 * (height // 16), 16 * (width // 16))
        if init_upscale:
            init_image = self.upscale(init_image)[0]
        return init_image

    def _pixels_out(self, img_px: torch.Tensor, output_type: str, jpeg_quality: int, upscale: bool = False, jpeg_encoder: str = "pil"):
        """decoded pixels -> what the request returns: the uint8 array or its JPEG, through the upscaler first when asked.  jpeg_encoder
        "native" (an encoder name already checked; ignored unless a JPEG is returned): the pixels stay on the device up to the encoder."""
        if jpeg_encoder == "native" and output_type == "jpeg":
            px = self.to_uint8_device(img_px)
            if upscale:
                px = self._require_upscaler().upscale_uint8_device(px)
            return self._jpeg_native(px, jpeg_quality)
        px = self.to_uint8(img_px)
        if upscale:
            px = self.upscale(px)
        return px if output_type == "uint8" else self._jpeg(px, jpeg_quality)

    @staticmethod
    def _jpeg(px: torch.Tensor, jpeg_quality: int = 99) -> io.BytesIO:
        from PIL import Image

        imgs = [px[i].numpy() for i in range(px.shape[0])]
        im = imgs[0] if len(imgs) == 1 else np.vstack(imgs)
        buf = io.BytesIO()
        Image.fromarray(im).save(buf, format="JPEG", quality=jpeg_quality)
        buf.seek(0)
        return buf

    # ---- loading (reference flux_pipeline.py:665-729) -------------------------------------------------------------------------
    @classmethod
    def load_pipeline_from_config_path(cls, path: str, flow_model_path: str = None, debug: bool = False, **kwargs) -> "FluxPipeline":
        with torch.inference_mode():
            config = load_config_from_path(path)
            if flow_model_path:
                config.ckpt_path = flow_model_path
            extra = {k: kwargs.pop(k, None) for k in ("state_dict", "ae_state_dict", "clip_kwargs", "t5_kwargs")}
            for k, v in kwargs.items():
                if hasattr(config, k):
                    setattr(config, k, v)
            return cls.load_pipeline_from_config(config, debug=debug, **extra)

    @classmethod
    def load_pipeline_from_config(cls, config: ModelSpec, debug: bool = False, state_dict=None, ae_state_dict=None, clip_kwargs=None,
                                  t5_kwargs=None) -> "FluxPipeline":
        """`state_dict` / `ae_state_dict` / `clip_kwargs` / `t5_kwargs` are offline hooks (weights, HF configs and tokenizers handed over in
        memory instead of read from the config's paths)."""
        from float8_quantize import quantize_flow_transformer_and_dispatch_float8

        with torch.inference_mode():
            models = load_models_from_config(config, state_dict=state_dict, ae_state_dict=ae_state_dict, clip_kwargs=clip_kwargs,
                                             t5_kwargs=t5_kwargs)
            redux = models.redux
            config = models.config
            flux_device = into_device(config.flux_device)
            # every shipped reference JSON says flow_dtype float16: accepted -- the engine computes in bf16 and the pipeline keeps the
            # configured dtype for what crosses its boundary (util.engine_flow_dtype; warned once)
            flux_dtype = into_dtype(config.flow_dtype)
            flow_model = models.flow
            if not config.prequantized_flow:
                flow_model = quantize_flow_transformer_and_dispatch_float8(
                    flow_model, flux_device, offload_flow=config.offload_flow, swap_linears_with_cublaslinear=False,
                    flow_dtype=engine_flow_dtype(config.flow_dtype), quantize_modulation=config.quantize_modulation,
                    quantize_flow_embedder_layers=config.quantize_flow_embedder_layers)
            else:
                flow_model.eval().requires_grad_(False)
        return cls(name=config.version, clip=models.clip, t5=models.t5, model=flow_model, ae=models.ae, dtype=flux_dtype, verbose=False,
                   flux_device=flux_device, ae_device=into_device(config.ae_device), clip_device=into_device(config.text_enc_device),
                   t5_device=into_device(config.text_enc_device), config=config, debug=debug, redux=redux,
                   controlnet=load_controlnet(config, device=flux_device), ip_adapter=load_ip_adapter(config, device=flux_device),
                   upscaler=load_upscaler(config, device=into_device(config.ae_device)),
                   depth_model=load_depth_model(config, device=into_device(config.ae_device)))
