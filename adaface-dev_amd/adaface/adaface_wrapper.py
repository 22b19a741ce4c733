"""Host-side mirror of the SD-1.5 ``text2img`` branch of the reference's ``adaface/adaface_wrapper.py`` (BASELINE configs[1],
the AdaFace inference path): ``AdaFaceWrapper.extend_tokenizer_and_text_encoder`` (:414-458), ``update_text_encoder_subj_embeddings``
(:461-489), ``update_prompt`` (:491-532), ``prepare_adaface_embeddings`` (:541-569), ``encode_prompt`` (:671-727) and ``forward``
(:730-809), with the same argument names and meaning.

The reference drives a diffusers ``StableDiffusionPipeline``; here the same steps run on this package's components -- the CLIP text
transformer (``CLIPTextModelWrapper``), ``LatentDiffusion`` + ``DDIMSampler`` (50 DDIM steps, (cond, uncond) CFG batches of 2 x
out_image_count, fused guidance + DDIM update) -- all through the gfx950 C ABI.  Offline there are no checkpoints, CLIP BPE vocabulary
files or VAE weights, so every component can be passed in, and:

* ``tokenizer``: any object with the transformers tokenizer protocol (``add_tokens``, ``convert_tokens_to_ids``, ``__len__``,
  ``__call__(..., padding="max_length", max_length=, truncation=True, return_tensors="pt").input_ids``), e.g.
  ``transformers.CLIPTokenizer.from_pretrained(local_dir)``.  The fallback ``WordTokenizer`` is a deterministic word-level stand-in
  (NOT CLIP BPE) so that synthetic-weight runs and tests exercise the same token-registration / prompt-rewriting logic;
* ``vae``: optional object with ``decode(latents / 0.18215) -> images in [-1, 1]`` (VAE decode is SURVEY.md 8f rank 3); without it
  ``forward`` returns the final latents ``[BS, 4, 64, 64]`` instead of PIL images.

Image sizes (INTEGRATION.md "Image sizes"): all three pipelines take any image whose sides are multiples of 64 from 64 to 1024 pixels
(latent sides multiples of 8 up to 128; ``text2img`` takes the size from ``noise``).  The VAE's attention layer runs fused
(``af_vae_attention``) wherever its three-launch form does not apply, and ``_to_pil`` decodes in slices of images when a batch would pass the
kernels' 32-bit activation bounds.  A larger side is a ValueError before any GPU work.

``pipeline_name="img2img"`` is the reference's img2img branch (diffusers' ``StableDiffusionImg2ImgPipeline`` with the DDIM scheduler,
what ``adaface_translate.py`` runs): ``forward``'s first argument carries the input image(s) (one PIL image or a list of 1 or
``out_image_count``; see ``img2img_images_u8``), ``vae`` must be an ``AutoencoderKL`` (encoder + decoder), and ``ref_img_strength``
picks how many of the last steps of the schedule run (``DDIMSampler.img2img_steps``).  The images are encoded once
(``LatentDiffusion.img2img_latents``: two fused kernels around the VAE encoder) and denoised by ``DDIMSampler.sample_img2img``
(``DPMSolverSampler.sample_img2img`` under ``"dpm++"``).

``pipeline_name="inpaint"`` is diffusers' ``StableDiffusionInpaintPipeline`` in its 4-channel U-Net branch (the SD-1.5 base model;
INTEGRATION.md "Inpainting"): img2img's input images and ``ref_img_strength``, plus ``forward``'s ``mask_image`` (one PIL image or a
list of 1 or ``out_image_count``; white = repaint; see ``inpaint_masks``).  It needs ``vae`` (an ``AutoencoderKL``) or
``base_model_path`` at construction, else ``InpaintVAEMissing``.  The images are encoded once
(``LatentDiffusion.inpaint_latents``) and ``sample_inpaint`` runs the img2img steps of the chosen sampler; after each step, in the
same kernel, the latent outside the mask is replaced by the image latent noised to the next timestep (the image latent itself after
the last step).

``default_scheduler_name="dpm++"`` (the reference's DPM-Solver++ scheduler, diffusers' ``DPMSolverSinglestepScheduler`` with its
defaults; INTEGRATION.md "DPM-Solver++ scheduler") samples both pipelines with ``DPMSolverSampler`` instead of ``DDIMSampler``: the same
(cond, uncond) batches and guidance rule, one fused guidance + DPM-Solver++ update per step, typically at 20-25 ``num_inference_steps``
rather than 50.  ``"ddim"`` stays the default.

``use_lcm=True, lcm_lora_path=...`` (the reference's LCM-LoRA mode; INTEGRATION.md "LCM-LoRA") fuses an SD-1.5 U-Net LoRA such as
LCM-LoRA into the U-Net weights once (``adaface/sd_lora.py``; after ``base_model_path`` is loaded, again after every later
``load_base_model``) and samples both pipelines with ``LCMSampler``, typically at 4 ``num_inference_steps``: the guidance scale is
constant, the (cond, uncond) batch runs only when the scale is above 1, and ``forward``'s ``generator`` draws the re-noising of every
step but the last.  Nothing is downloaded: ``lcm_lora_path`` is a local file or an in-memory state dict.  ``fuse_lcm_lora`` /
``unfuse_lcm_lora`` change the weights only; the sampler follows ``use_lcm``.

``forward(..., hires_size=(W, H))`` (``text2img`` only; INTEGRATION.md "High-resolution text2img") samples in two passes, under any
of the three samplers: the usual run at the size of ``noise``, then ``LatentDiffusion.hires_latents`` (one fused kernel: the latents
resampled to the target size, ``hires_upscaler`` "bilinear" or "bicubic", and noised to the second pass's first timestep) and
``sample_img2img`` over ``hires_strength`` of ``hires_steps`` (default ``num_inference_steps``) at the target size.  Antialiased,
nearest and pixel-space upscalers between the passes, hires for img2img / inpaint and graph capture of the two passes are not built
(model-based upscaling of the final images is ``upscale=True``, below).

``forward(noise, prompt, out_image_count=V, num_frames=F)`` (``text2img`` only; INTEGRATION.md "Video (motion modules)") generates V
clips of F frames with an AnimateDiff motion module (``motion_module_path`` / ``load_motion_module``, a local ``.ckpt`` / ``.pth`` file
or its state dict; ``ldm/modules/motion_module.py``): ``noise`` is ``[V * F, 4, h, w]`` video-major, the prompt is repeated per frame,
the module sits on the U-Net during the sampling call only, and V lists of F images come back (the latents without a ``vae``).
``beta_schedule="sqrt_linear"`` gives the plain-linear betas AnimateDiff's configs use.  Training, MotionLoRA, SparseCtrl, sliding
context windows, img2video, the diffusers MotionAdapter layout and GIF / MP4 writing are not built.

``forward(..., upscale=True)`` (INTEGRATION.md "Upscaling (Real-ESRGAN)") sends the quantised images of every pipeline -- ``hires_size``
results, the frames of a video and the pasted-back photo of the repaint path included -- through a Real-ESRGAN ``Upscaler``
(``upscaler=`` at construction or ``load_upscaler``: an ``Upscaler``, an ``RRDBNet`` or a local ``.pth`` file; adaface/esrgan.py) on the
device before they become PIL images.  Without a loaded upscaler, without a ``vae``, or for a result above the upscaler's 1024-pixel
input limit it is a ValueError before any GPU work.  ``upscale=False`` is the call as it was.

``forward(..., restore_faces=True)`` (INTEGRATION.md "Face restoration (GFPGAN)") sends the same quantised images through a GFPGAN
``FaceRestorer`` (``face_restorer=`` at construction or ``load_face_restorer``; adaface/gfpgan.py) on the device, BEFORE the upscaler and
before they become PIL images: every detected face is aligned, restored and pasted back with a soft border.  Without a loaded restorer or
without a ``vae`` it is a ValueError before any GPU work.  ``restore_faces=False`` is the call as it was.

``forward(..., control_image=img, control_scale=1.0, control_guidance_start=0.0, control_guidance_end=1.0)`` (INTEGRATION.md
"ControlNet") steers all three pipelines, under all three samplers and with ``num_frames``, with a ControlNet (``controlnet=`` at
construction or ``load_controlnet``: a ``ControlNet`` or a local cldm-layout file / state dict;
ldm/modules/diffusionmodules/controlnet.py).  ``control_image`` is a PIL image, a uint8 tensor ``[H, W, 3]`` / ``[B, H, W, 3]`` or a list,
1 image (shared) or one per sampled row, exactly 8 x the latent size.  The hints are encoded once, the ControlNet sits on the U-Net during
the sampling call only, and the sampler's per-step callback switches it by the guidance window.  Without ``control_image`` every path is
the call as it was.

``forward(..., ip_adapter_image=img | ip_adapter_face_id=emb, ip_adapter_scale=1.0, ip_guidance_start=0.0, ip_guidance_end=1.0)``
(INTEGRATION.md "IP-Adapter") adds an image prompt on all three pipelines, under all three samplers, with ``num_frames``, ``control_image``
and both passes of ``hires_size``, with an IP-Adapter or IP-Adapter-FaceID (``ip_adapter=`` / ``ip_image_encoder=`` at construction or
``load_ip_adapter``: an ``IPAdapter`` or a local published file / state dict; adaface/ip_adapter.py).  ``ip_adapter_image`` is a PIL image,
a path, or uint8 ``[H, W, 3]`` / ``[B, H, W, 3]``, 1 (shared) or one per sampled row; for a FaceID adapter the id is extracted from it by the
``face_id_extractor``, or given as ``ip_adapter_face_id`` fp ``[1 | rows, 512]``.  The tokens are computed once, the adapter sits on the
U-Net during the sampling call only, and the sampler's per-step callback switches it by its guidance window.  A FaceID file's LoRA is fused
into the U-Net's weights while the adapter is loaded (``unload_ip_adapter`` restores them).  Without these arguments every path is the call
as it was.

``forward(..., region_masks=[m1, m2], region_prompts=[p1, p2] | region_prompt_embeds=[e1, e2], region_base_weight=0.2)`` (INTEGRATION.md
"Regional prompts / several subjects") composes several prompts -- and, through ``region_prompt_embeds``, several subjects -- in one picture
on all three pipelines, under all three samplers, with ``control_image`` and with an IP-Adapter: every cross-attention layer attends to the
base prompt and to each region's prompt and blends the results per token under the masks (PIL "L" images, uint8 arrays or tensors of the
image's size, white = the region), area-averaged onto the layer's token grid: ``w_r = (1 - beta) m_r / max(1, s)``, the base prompt keeps
``beta + (1 - beta)(1 - min(1, s))`` (``ops.region_weights``, ``ops.region_attention``: one launch per layer, a region's K / V are not read
where it has no weight).  The unconditional half runs the negative prompt alone.  The regions sit on the U-Net during the sampling call only
(``UNetModel.set_regions``).  Not built: regions with ``num_frames``, ``hires_size`` or ``crop_padding``.  Without these arguments every
path is the call as it was.

``forward(photo, ..., mask_image="face", crop_padding=0.5)`` (``inpaint`` only; INTEGRATION.md "Repainting faces in a photo") repaints
the faces of ONE photo of any size (a PIL image, a path or a uint8 array) and hands back the same photo: ``face_detector`` (any callable
with ``FaceIDExtractor``'s detector contract, e.g. a ``RetinaFaceDetector``; by default the ``face_id_extractor``'s) finds the faces,
``ops.face_alpha_mask`` draws a soft elliptical mask on the device (``face_mask_expand``, ``face_mask_feather``; ``face_index=k`` keeps
the k-th face only), ``face_repaint.crop_region`` picks a padded rectangle around them, ``ops.crop_resize_u8`` resamples it to
``work_size`` (default 512 x 512) and derives the latent mask, the inpaint machinery above runs unchanged, and ``ops.paste_back_u8``
resamples the decoded crop back, blends it into the photo under the soft mask and quantises, in one launch.  Pixels that are not
repainted come back bit-identical.  ``crop_padding=None`` with ``"face"`` runs the whole photo (through ``img2img_images_u8``'s size
rules) and pastes back, so unmasked pixels are exact; a PIL mask with ``crop_padding`` runs the crop path under the hard mask v >= 128
around the mask's bounding box; a PIL mask without ``crop_padding`` is the plain inpaint path above.  Still not built: one pass per
face, Gaussian-blurred user masks, 9-channel inpainting U-Nets and graph capture of the loop.

SDXL / SD3 / flux pipelines, LCM-distilled U-Nets, schedulers other than DDIM, DPM-Solver++ and LCM, U-Net ensembles and the
ConsistentID encoder are out of scope (external packages).  Of inpainting, 9-channel inpainting U-Nets, caller-supplied
``masked_image_latents`` and graph capture of the loop are not built."""
import re
import zlib

import numpy as np
import torch
import torch.nn as nn

from .. import SD15_UNET_CONFIG, ops
from ..ldm.models.diffusion.ddim import DDIMSampler
from ..ldm.models.diffusion.ddpm import LatentDiffusion
from ..ldm.models.diffusion.dpm_solver import DPMSolverSampler
from ..ldm.models.diffusion.lcm import LCMSampler, lcm_timesteps
from . import face_repaint, sd_lora
from .arc2face_models import CLIPTextModelWrapper, clip_text_config
from .face_align import load_rgb_u8
from .face_id_to_ada_prompt import Arc2Face_ID2AdaPrompt
from .face_repaint import FaceDetectorMissing, NoFaceFound      # noqa: F401  (re-exported: what forward(mask_image="face") raises)
from .subj_basis_generator import CLIP_BOS, CLIP_EOS, CLIP_IDS


def img2img_images_u8(images, out_image_count):
    """img2img input preparation on the host: one PIL image or a list of 1 or ``out_image_count`` images, all of one size, converted
    to RGB; a side that is not a multiple of 64 is resized down to one (LANCZOS; the U-Net needs a latent divisible by 8).
    Returns uint8 [B_img, H, W, 3] on the CPU."""
    from PIL import Image
    imgs = list(images) if isinstance(images, (list, tuple)) else [images]
    if len(imgs) not in (1, out_image_count):
        raise ValueError(f"img2img takes 1 or out_image_count = {out_image_count} input images, got {len(imgs)}")
    for im in imgs:
        if not isinstance(im, Image.Image):
            raise ValueError(f"img2img input images must be PIL images, got {type(im).__name__}")
    sizes = {im.size for im in imgs}
    if len(sizes) != 1:
        raise ValueError(f"img2img input images must all have the same size, got {sorted(sizes)}")
    w, h = imgs[0].size
    if w < 64 or h < 64:
        raise ValueError(f"img2img input images must be at least 64 x 64 pixels, got {w} x {h}")
    w64, h64 = w // 64 * 64, h // 64 * 64
    arrs = []
    for im in imgs:
        im = im.convert("RGB")
        if (w64, h64) != (w, h):
            im = im.resize((w64, h64), resample=Image.LANCZOS)
        arrs.append(np.asarray(im, dtype=np.uint8))
    return torch.from_numpy(np.stack(arrs))


def inpaint_masks(mask_images, out_image_count, size):
    """Inpainting mask preparation on the host: one PIL image or a list of 1 or ``out_image_count`` images, each converted to "L" and
    resized (LANCZOS) to ``size`` = (W, H) of the prepared input images when it differs.  White means repaint: m = v >= 128
    (v / 255 >= 0.5) at full resolution, then nearest-neighbour to the latent grid, m_lat[i, j] = m[8 i, 8 j].
    Returns fp32 {0, 1} [B_mask, 1, H/8, W/8] on the CPU."""
    from PIL import Image
    masks = list(mask_images) if isinstance(mask_images, (list, tuple)) else [mask_images]
    if len(masks) not in (1, out_image_count):
        raise ValueError(f"inpainting takes 1 or out_image_count = {out_image_count} mask images, got {len(masks)}")
    out = []
    for im in masks:
        if not isinstance(im, Image.Image):
            raise ValueError(f"inpainting mask images must be PIL images, got {type(im).__name__}")
        im = im.convert("L")
        if im.size != tuple(size):
            im = im.resize(tuple(size), resample=Image.LANCZOS)
        out.append(np.asarray(im, dtype=np.uint8)[::8, ::8] >= 128)
    return torch.from_numpy(np.stack(out)[:, None].astype(np.float32))


def control_images_u8(control_image, rows):
    """ControlNet input preparation on the host: a PIL image, a uint8 tensor [H, W, 3] / [B, H, W, 3] or a list of either, 1 (shared by all
    rows) or ``rows`` of them, all of one size.  Nothing is resized.  Returns uint8 [B_ctl, H, W, 3] (on the device the tensors were on)."""
    from PIL import Image
    items = list(control_image) if isinstance(control_image, (list, tuple)) else [control_image]
    out = []
    for im in items:
        if isinstance(im, Image.Image):
            out.append(torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy()))
        elif torch.is_tensor(im) and im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3:
            out.append(im)
        elif torch.is_tensor(im) and im.dtype == torch.uint8 and im.dim() == 4 and im.shape[3] == 3:
            out.extend(im)
        else:
            raise ValueError("control_image must be a PIL image, a uint8 tensor [H, W, 3] / [B, H, W, 3] or a list of them, got "
                             f"{(im.dtype, tuple(im.shape)) if torch.is_tensor(im) else type(im).__name__}")
    if len(out) not in (1, rows):
        raise ValueError(f"control_image: 1 image (shared) or one per sampled row ({rows}) expected, got {len(out)}")
    sizes = {tuple(t.shape[:2]) for t in out}
    if len(sizes) != 1:
        raise ValueError(f"control images must all have the same size, got {sorted(sizes)}")
    return torch.stack(out)


MAX_IMAGE_SIDE = 1024      # pixels; the VAE (its fused attention layer, 16384 tokens) is built and tested up to a 128 x 128 latent


# default_scheduler_name -> sampler class (a sampling.Sampler, as LCMSampler: sample / img2img_steps / sample_img2img)
SCHEDULERS = {"ddim": DDIMSampler, "dpm++": DPMSolverSampler}


class InpaintVAEMissing(ValueError, NotImplementedError):
    """``pipeline_name="inpaint"`` with neither ``vae`` nor ``base_model_path``: nothing to encode the input images with.  A
    ValueError; also a NotImplementedError, which is what ``pipeline_name="inpaint"`` raised before inpainting was built, so callers
    that caught that keep working."""


class LCMLoRAMissing(ValueError, NotImplementedError):
    """``use_lcm=True`` without ``lcm_lora_path``.  A ValueError; also a NotImplementedError, which is what ``use_lcm=True`` raised
    before LCM sampling was built, so callers that caught that keep working."""


class WordTokenizer:
    """Deterministic word-level tokenizer with the CLIP special ids (BOS 49406, EOS = pad 49407) -- a stand-in for CLIP BPE."""

    def __init__(self, vocab_size=49408):
        self.base_vocab = vocab_size
        self.added = {}

    def __len__(self):
        return self.base_vocab + len(self.added)

    def add_tokens(self, tokens):
        n = 0
        for t in tokens:
            if t not in self.added:
                self.added[t] = self.base_vocab + len(self.added)
                n += 1
        return n

    def convert_tokens_to_ids(self, tokens):
        one = isinstance(tokens, str)
        ids = [self._id(t) for t in ([tokens] if one else tokens)]
        return ids[0] if one else ids

    def _id(self, w):
        if w in self.added:
            return self.added[w]
        if w in CLIP_IDS:
            return CLIP_IDS[w]
        return 1 + zlib.crc32(w.encode()) % (CLIP_BOS - 1)

    def tokenize(self, text):
        return re.findall(r"[A-Za-z0-9_]+|[^\sA-Za-z0-9_]", text.lower() if not self.added else self._lower_keep_added(text))

    def _lower_keep_added(self, text):
        return " ".join(w if w in self.added else w.lower() for w in text.split())

    def __call__(self, texts, padding="max_length", max_length=77, truncation=True, return_tensors="pt", **unused):
        texts = [texts] if isinstance(texts, str) else list(texts)
        rows = []
        for t in texts:
            ids = [CLIP_BOS] + [self._id(w) for w in self.tokenize(t)][:max_length - 2] + [CLIP_EOS]
            rows.append(ids + [CLIP_EOS] * (max_length - len(ids)))
        return _Encoding(input_ids=torch.tensor(rows, dtype=torch.long))


class _Encoding(dict):
    """transformers' BatchEncoding protocol: enc["input_ids"] and enc.input_ids."""
    __getattr__ = dict.__getitem__


class AdaFaceWrapper(nn.Module):
    def __init__(self, pipeline_name="text2img", base_model_path=None, adaface_encoder_types=("arc2face",), adaface_ckpt_paths=None,
                 adaface_encoder_cfg_scales=None, enabled_encoders=None, use_lcm=False, default_scheduler_name="ddim",
                 num_inference_steps=50, subject_string="z", negative_prompt=None, max_prompt_length=77,
                 enable_static_img_suffix_embs=None, device="cuda", is_training=False,
                 tokenizer=None, text_encoder=None, ldm=None, vae=None, id2ada_prompt_encoder=None, unet_config=None, clip_config=None,
                 lcm_lora_path=None, lcm_lora_scale=1.0, face_id_extractor=None, face_detector=None, motion_module_path=None,
                 beta_schedule="linear", upscaler=None, face_restorer=None, controlnet=None, ip_adapter=None, ip_image_encoder=None, freeu=None):
        super().__init__()
        if pipeline_name not in ("text2img", "img2img", "inpaint", None):
            raise NotImplementedError(f"pipeline {pipeline_name!r}: only the SD-1.5 text2img, img2img and inpaint paths (and None = face "
                                      "encoder only) are built")
        if pipeline_name == "inpaint" and vae is None and base_model_path is None:
            raise InpaintVAEMissing("pipeline_name='inpaint' encodes its input images: pass vae (an AutoencoderKL, encoder + decoder) or "
                                    "base_model_path (whose VAE is loaded)")
        if list(adaface_encoder_types) != ["arc2face"]:
            raise NotImplementedError("only the Arc2Face ID encoder is in scope (ConsistentID needs an external package)")
        if default_scheduler_name not in SCHEDULERS:
            raise NotImplementedError(f"scheduler {default_scheduler_name!r}: only {' and '.join(map(repr, SCHEDULERS))} (and "
                                      "use_lcm=True) are built")
        if use_lcm:
            if pipeline_name is None:
                raise ValueError("use_lcm=True needs a pipeline: pipeline_name=None builds the face encoder only")
            if lcm_lora_path is None:
                raise LCMLoRAMissing("use_lcm=True needs lcm_lora_path (a local LCM-LoRA file such as the pytorch_lora_weights.safetensors "
                                     "of latent-consistency/lcm-lora-sdv1-5, or its state dict): nothing is downloaded")
            lcm_timesteps(num_inference_steps)          # 1 .. 50 steps, else ValueError
        elif lcm_lora_path is not None:
            raise ValueError("lcm_lora_path is given but use_lcm is False")
        self.pipeline_name = pipeline_name
        self.use_lcm = use_lcm
        self.default_scheduler_name = default_scheduler_name
        self.adaface_encoder_types = list(adaface_encoder_types)
        self.adaface_ckpt_paths = adaface_ckpt_paths
        self.enabled_encoders = enabled_encoders
        self.enable_static_img_suffix_embs = enable_static_img_suffix_embs
        self.subject_string = subject_string
        self.num_inference_steps = num_inference_steps
        self.max_prompt_length = max_prompt_length
        self.device = device
        self.is_training = is_training
        self.negative_prompt = negative_prompt if negative_prompt is not None else (
            "flaws in the eyes, flaws in the face, lowres, non-HDRi, low quality, worst quality, artifacts, noise, text, watermark, glitch, "
            "mutated, ugly, disfigured, hands, partially rendered objects, partially rendered eyes, deformed eyeballs, cross-eyed, blurry, "
            "mutation, duplicate, out of frame, cropped, mutilated, bad anatomy, deformed, bad proportions, "
            "nude, naked, nsfw, topless, bare breasts")
        ccfg = clip_config or clip_text_config()
        self.tokenizer = tokenizer or WordTokenizer(ccfg.vocab_size)
        self.text_encoder = text_encoder or CLIPTextModelWrapper(ccfg)
        # face_id_extractor (adaface/face_align.py FaceIDExtractor): prepare_adaface_embeddings(image_paths) then extracts the IDs itself
        self.id2ada_prompt_encoder = id2ada_prompt_encoder or Arc2Face_ID2AdaPrompt(clip_config=ccfg, face_id_extractor=face_id_extractor)
        if face_id_extractor is not None and id2ada_prompt_encoder is not None:
            id2ada_prompt_encoder.face_id_extractor = face_id_extractor
        if adaface_encoder_cfg_scales is not None:
            self.id2ada_prompt_encoder.out_id_embs_cfg_scale = adaface_encoder_cfg_scales[0]
        self.encoders_num_id_vecs = [self.id2ada_prompt_encoder.num_id_vecs]
        # forward(mask_image="face"): any callable with FaceIDExtractor's detector contract; by default the extractor's own
        self.face_detector = face_detector if face_detector is not None else getattr(face_id_extractor, "detect_faces", None)
        if ldm is not None and beta_schedule != "linear":
            raise ValueError("beta_schedule is given together with a ready ldm: build that LatentDiffusion with the schedule instead")
        # beta_schedule: make_beta_schedule's names -- "linear" is SD's scaled-linear table, "sqrt_linear" the plain-linear betas of AnimateDiff's configs
        self.ldm = None if pipeline_name is None else (ldm or LatentDiffusion(unet_config or SD15_UNET_CONFIG, beta_schedule=beta_schedule))
        self.__dict__["upscaler"] = None          # an esrgan.Upscaler (load_upscaler) for forward(upscale=True); not a submodule
        self.__dict__["face_restorer"] = None     # a gfpgan.FaceRestorer (load_face_restorer) for forward(restore_faces=True); not a submodule
        self.__dict__["motion_module"] = None     # a MotionModule (load_motion_module); not a submodule: it is on the U-Net only inside forward(num_frames=F)
        self.__dict__["controlnet"] = None        # a ControlNet (load_controlnet); not a submodule: it is on the U-Net only inside forward(control_image=...)
        self.__dict__["ip_adapter"] = None        # an IPAdapter (load_ip_adapter); not a submodule: it is on the U-Net only inside forward(ip_adapter_image= / ip_adapter_face_id=)
        self.__dict__["freeu"] = None             # enable_freeu's values ({"b1", "b2", "s1", "s2", "version"}) while FreeU is on; they live on the U-Net (set_freeu)
        self.__dict__["ip_image_encoder"] = None  # the CLIP ViT-H/14 VisionTransformer of a kind="clip" adapter; not a submodule
        self.vae = vae
        self.img_prompt_embs = None
        self._lcm_lora = None                 # (read_unet_lora dict, scale) of the fused LoRA
        self._lcm_saved = {}                  # {ldm_path: original weight} while it is fused
        if base_model_path is not None:
            self.load_base_model(base_model_path)
        if use_lcm:
            self.fuse_lcm_lora(lcm_lora_path, lcm_lora_scale)
        self.extend_tokenizer_and_text_encoder()
        if adaface_ckpt_paths:
            self.load_subj_basis_generator(adaface_ckpt_paths)
        if motion_module_path is not None:
            self.load_motion_module(motion_module_path)
        if upscaler is not None:
            self.load_upscaler(upscaler)
        if face_restorer is not None:
            self.load_face_restorer(face_restorer)
        if controlnet is not None:
            self.load_controlnet(controlnet)
        if ip_adapter is not None:
            self.load_ip_adapter(ip_adapter, ip_image_encoder)
        elif ip_image_encoder is not None:
            raise ValueError("ip_image_encoder is given without ip_adapter")
        if freeu is not None and freeu is not False:
            if freeu is True:
                self.enable_freeu()
            elif isinstance(freeu, dict):
                unknown = sorted(set(freeu) - {"b1", "b2", "s1", "s2", "version"})
                if unknown:
                    raise ValueError(f"freeu: unknown key(s) {unknown}: expected b1, b2, s1, s2, version")
                self.enable_freeu(**freeu)
            else:
                raise ValueError(f"freeu must be None, True or a dict(b1=, b2=, s1=, s2=, version=), got {type(freeu).__name__}")

    # ------------------------------------------------------------------ checkpoints
    def load_base_model(self, base_model_path):
        """An LDM-format SD-1.5 checkpoint (.safetensors / .ckpt): U-Net, VAE and CLIP text encoder by their key prefixes
        (the reference hands the same file to diffusers' ``from_single_file``, adaface_wrapper.py:236-246, 301-308)."""
        from ..ldm.modules.encoders.modules import FrozenCLIPEmbedder
        if self.ldm is None:
            raise RuntimeError("pipeline_name=None builds the face encoder only: there is no U-Net to load a base model into")
        if self.ldm.first_stage_model is None:
            self.ldm.instantiate_first_stage()
        if self.ldm.cond_stage_model is None:       # share the wrapper's text encoder so that the checkpoint's CLIP weights reach it
            self.ldm.instantiate_cond_stage(FrozenCLIPEmbedder(tokenizer=self.tokenizer, transformer=self.text_encoder,
                                                               last_layers_skip_weights=None))
        if self._lcm_saved:                   # the checkpoint goes into the unfused weights, the LoRA is fused again onto it
            sd_lora.unfuse_unet_lora(self.ldm.model, self._lcm_saved)
            self._lcm_saved = {}
        missing, unexpected = self.ldm.init_from_ckpt(base_model_path)
        if self.vae is None:
            self.vae = self.ldm.first_stage_model
        if self._lcm_lora is not None:
            self._lcm_saved = sd_lora.fuse_unet_lora(self.ldm.model, *self._lcm_lora)
        return missing, unexpected

    def load_motion_module(self, path_or_state_dict):
        """An AnimateDiff motion module (a local ``.ckpt`` / ``.pth`` file or its state dict; ldm/modules/motion_module.py) for
        ``forward(..., num_frames=F)``.  Strict: a file that does not match raises ValueError.  Nothing is downloaded."""
        from ..ldm.modules.motion_module import MotionModule
        if self.ldm is None:
            raise RuntimeError("pipeline_name=None builds the face encoder only: there is no U-Net to put a motion module on")
        mm = MotionModule(path_or_state_dict)
        self.ldm.model.diffusion_model.set_motion(mm, 1)        # refuses widths that do not match this U-Net
        self.ldm.model.diffusion_model.set_motion(None)
        self.__dict__["motion_module"] = mm
        return mm

    def unload_motion_module(self):
        self.__dict__["motion_module"] = None
        if self.ldm is not None:
            self.ldm.model.diffusion_model.set_motion(None)

    def enable_freeu(self, s1=0.9, s2=0.2, b1=1.5, b2=1.6, version=2):
        """FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net"; INTEGRATION.md "FreeU") for every later ``forward``: the decoder's
        backbone features are boosted (b1 / b2) and its skip features lose part of their lowest spatial frequencies (s1 / s2), in the two
        stages whose backbone has 4 x / 2 x ``model_channels`` channels.  Argument order and names are diffusers' ``enable_freeu``; the
        defaults are the authors' values for SD-1.5.  ``version=1`` boosts by the constant b instead of the per-pixel map.  It works on all
        pipelines and samplers and beside ``num_frames``, ``control_image``, an IP-Adapter, regions, both passes of ``hires_size`` and face
        repainting: every U-Net call of the wrapper goes through the walk that applies it.  Bad values are a ValueError naming the
        argument, before any GPU work."""
        from ..ldm.modules.diffusionmodules.openaimodel import check_freeu_values
        if self.ldm is None:
            raise RuntimeError("pipeline_name=None builds the face encoder only: there is no U-Net to run FreeU in")
        cfg = check_freeu_values("enable_freeu", b1, b2, s1, s2, version)
        self.ldm.model.diffusion_model.set_freeu(**cfg)
        self.__dict__["freeu"] = cfg
        return cfg

    def disable_freeu(self):
        self.__dict__["freeu"] = None
        if self.ldm is not None:
            self.ldm.model.diffusion_model.set_freeu(None)

    def load_controlnet(self, path_or_net):
        """A ControlNet for ``forward(..., control_image=...)`` (ldm/modules/diffusionmodules/controlnet.py; INTEGRATION.md "ControlNet"): a
        ``ControlNet``, or a local cldm-layout ``.pth`` / ``.ckpt`` / ``.safetensors`` file or its state dict, loaded strictly for this
        wrapper's U-Net.  Nothing is downloaded."""
        from ..ldm.modules.diffusionmodules.controlnet import ControlNet, load_controlnet
        if self.ldm is None:
            raise RuntimeError("pipeline_name=None builds the face encoder only: there is no U-Net to put a ControlNet on")
        unet = self.ldm.model.diffusion_model
        cn = path_or_net
        if not isinstance(cn, ControlNet):
            cfg = dict(in_channels=unet.in_channels, model_channels=unet.model_channels, num_res_blocks=unet.num_res_blocks,
                       attention_resolutions=unet.attention_resolutions, channel_mult=unet.channel_mult, num_heads=unet.num_heads,
                       num_head_channels=unet.num_head_channels, use_spatial_transformer=True,
                       context_dim=unet._cross_attn_layers()[0].to_k.in_features)
            cn = load_controlnet(cn, cfg)
        probe = torch.zeros((1, 1, 1, unet.model_channels), dtype=torch.float16)
        unet.set_control(cn, probe)                              # refuses widths or a topology that do not match this U-Net
        unet.set_control(None)
        self.__dict__["controlnet"] = cn
        return cn

    def unload_controlnet(self):
        self.__dict__["controlnet"] = None
        if self.ldm is not None:
            self.ldm.model.diffusion_model.set_control(None)

    def _check_control(self, control_image, control_scale, start, end, rows, hires_size, repaint):
        """The refusals of forward(control_image=...) that need no image size (INTEGRATION.md "ControlNet"), all before any GPU work.  Returns
        the control images as uint8 [1 | rows, H, W, 3]."""
        if self.controlnet is None:
            raise ValueError("control_image is given but no ControlNet is loaded (controlnet= at construction / load_controlnet)")
        if hires_size is not None:
            raise ValueError("control_image together with hires_size: the second pass runs at another size and resampling hints is not built")
        if repaint is not None:
            raise ValueError("control_image together with mask_image='face' or crop_padding: the working size is chosen under the hint and "
                             "resampling hints is not built")
        if isinstance(control_scale, bool) or not isinstance(control_scale, (int, float)) or not np.isfinite(control_scale):
            raise ValueError(f"control_scale must be a finite number, got {control_scale!r}")
        ok = all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in (start, end))
        if not ok or not 0 <= start < end <= 1:
            raise ValueError(f"the control guidance window needs 0 <= control_guidance_start < control_guidance_end <= 1, got {start!r}, {end!r}")
        return control_images_u8(control_image, rows)

    @staticmethod
    def _check_control_size(images, latent_hw):
        if tuple(images.shape[1:3]) != (8 * latent_hw[0], 8 * latent_hw[1]):
            raise ValueError(f"control images must be exactly 8 x the latent size, {8 * latent_hw[1]} x {8 * latent_hw[0]} pixels, got "
                             f"{images.shape[2]} x {images.shape[1]} (nothing is resized)")

    def _sample_controlled(self, control, n_steps, call, ip=None, regions=None):
        """``call(**kw)`` runs one of the sampler's loops.  With ``control`` = (images uint8, scale, start, end) the ControlNet is on the
        U-Net around that call only: the hints are encoded once, and the sampler's per-step callback switches the control off and on by the
        guidance window (active at step i of n iff i / n >= start and (i + 1) / n <= end).  With ``ip`` = (cond tokens, uncond tokens, scale,
        start, end) the IP-Adapter is on the U-Net in the same way, under its own window.  Without either this is ``call()``: the sampler is
        called exactly as before.  With ``regions`` = (contexts, uncond context, level weights) the regional prompts are set on the U-Net around
        the call too (UNetModel.set_regions; no window)."""
        if control is None and ip is None and regions is None:
            return call()
        from ..ldm.modules.diffusionmodules.controlnet import guidance_window_active
        unet = self.ldm.model.diffusion_model

        def switch(i):
            if control is not None:
                unet.set_control_active(i < n_steps and guidance_window_active(i, n_steps, control[2], control[3]))
            if ip is not None:
                unet.set_ip_adapter_active(i < n_steps and guidance_window_active(i, n_steps, ip[3], ip[4]))

        try:
            if regions is not None:
                unet.set_regions(*regions)
            if control is not None:
                cn = self.controlnet.to(self.device)
                unet.set_control(cn, cn.hint_features(control[0].to(self.device)), control[1])
            if ip is not None:
                unet.set_ip_adapter(self.ip_adapter, ip[0], ip[1], ip[2])
            if control is None and ip is None:
                return call()
            switch(0)
            return call(callback=lambda i: switch(i + 1))                # the callback runs behind step i
        finally:
            unet.set_control(None)
            unet.set_ip_adapter(None)
            unet.set_regions(None)

    # ------------------------------------------------------------------ regional prompts (INTEGRATION.md "Regional prompts / several subjects")
    def _check_regions(self, masks, prompts, embeds, beta, num_frames, hires_size, crop_padding):
        """The refusals of forward(region_masks=...) that do not need the image size, all before any GPU work.  Returns the masks as one uint8
        array [R - 1, H, W] (white = the region)."""
        if masks is None:
            raise ValueError("region_prompts / region_prompt_embeds are given without region_masks")
        if (prompts is None) == (embeds is None):
            raise ValueError("regions need exactly one of region_prompts (strings) and region_prompt_embeds (encode_prompt results)")
        for name, v in (("num_frames", num_frames), ("hires_size", hires_size), ("crop_padding", crop_padding)):
            if v is not None:
                raise ValueError(f"regional prompts are not built with {name}")
        if torch.is_tensor(masks) or isinstance(masks, np.ndarray):
            masks = list(masks) if masks.ndim == 3 else [masks]
        if not isinstance(masks, (list, tuple)) or not masks:
            raise ValueError("region_masks must be a list of PIL 'L' images, uint8 arrays or tensors [H, W]")
        given = prompts if prompts is not None else embeds
        if not isinstance(given, (list, tuple)) or len(given) != len(masks):
            raise ValueError(f"{len(masks)} region masks but {len(given) if isinstance(given, (list, tuple)) else type(given).__name__} region prompts: "
                             "one prompt per mask")
        if len(masks) > ops.REGION_MAX - 1:
            raise ValueError(f"at most {ops.REGION_MAX - 1} regions (beside the base prompt), got {len(masks)}")
        if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not 0 <= beta <= 1:
            raise ValueError(f"region_base_weight must be in [0, 1], got {beta!r}")
        if prompts is not None and not all(isinstance(t, str) for t in prompts):
            raise ValueError("region_prompts must be strings")
        if embeds is not None and not all(isinstance(e, (list, tuple)) and len(e) in (2, 4) and torch.is_tensor(e[0]) and e[0].dim() == 3 for e in embeds):
            raise ValueError("region_prompt_embeds must hold one encode_prompt result (a 2- or 4-tuple of embeddings) per region")
        out = []
        for m in masks:
            if torch.is_tensor(m):
                m = m.detach().cpu().numpy()
            elif not isinstance(m, np.ndarray):
                m = np.asarray(m.convert("L")) if hasattr(m, "convert") else np.asarray(m)
            if m.dtype == np.bool_:
                m = m.astype(np.uint8) * 255
            if m.ndim != 2 or m.dtype != np.uint8:
                raise ValueError(f"a region mask must be a PIL 'L' image or uint8 [H, W] (255 = the region), got {m.dtype} {m.shape}")
            if out and m.shape != out[0].shape:
                raise ValueError(f"the region masks differ in size: {out[0].shape} and {m.shape}")
            out.append(m)
        return np.ascontiguousarray(np.stack(out, 0))

    @staticmethod
    def _check_region_size(masks_u8, hw):
        if hw[0] % 64 or hw[1] % 64:
            raise ValueError(f"regional prompts need an image whose sides are multiples of 64 pixels, got {hw[1]} x {hw[0]}")
        if tuple(masks_u8.shape[1:]) != tuple(hw):
            raise ValueError(f"the region masks must be the image's size, {hw[1]} x {hw[0]} pixels, got {masks_u8.shape[2]} x {masks_u8.shape[1]} "
                             "(nothing is resized)")

    def _region_state(self, masks_u8, prompts, embeds, beta, pe, ne, kw):
        """(contexts fp16 [rows, R, L, C], uncond context fp16 [rows, L, C], the levels' weights) for UNetModel.set_regions: set 0 is the base
        prompt ``pe`` [rows, L, C], the regions' prompts are encoded with the subject currently set."""
        if prompts is not None:
            embeds = [self.encode_prompt(t, None, device=self.device, **kw) for t in prompts]
        rows = pe.shape[0]
        sets = [pe] + [e[0].to(self.device).expand(rows, -1, -1) if e[0].shape[0] == 1 else e[0].to(self.device) for e in embeds]
        for t in sets[1:]:
            if tuple(t.shape) != tuple(pe.shape):
                raise ValueError(f"a region's prompt embeddings are {tuple(t.shape)}, the base prompt's {tuple(pe.shape)}")
        contexts = torch.stack([t.to(torch.float16) for t in sets], 1).contiguous()
        uncond = (pe if ne is None else ne).to(torch.float16).contiguous()
        _, levels = ops.region_weights(torch.from_numpy(masks_u8).to(self.device), float(beta))
        return contexts, uncond, levels

    # ------------------------------------------------------------------ IP-Adapter (adaface/ip_adapter.py; INTEGRATION.md "IP-Adapter")
    def load_ip_adapter(self, path_or_obj, image_encoder=None, lora_scale=1.0):
        """An IP-Adapter (``kind="clip"``) or IP-Adapter-FaceID (``kind="faceid"``) for ``forward(..., ip_adapter_image= / ip_adapter_face_id=)``:
        an ``IPAdapter``, or a local ``.bin`` / ``.safetensors`` file or its state dict, loaded strictly for this wrapper's U-Net.
        ``image_encoder``: the CLIP ViT-H/14 vision tower of a ``clip`` adapter -- a ``VisionTransformer``, or a local file / state dict in
        transformers' ``CLIPVisionModelWithProjection`` layout.  A FaceID file's LoRA is fused into the U-Net here (``lora_scale``) and
        unfused by ``unload_ip_adapter``.  Nothing is downloaded."""
        from . import ip_adapter as IP
        from ..evaluation import vit
        if self.ldm is None:
            raise RuntimeError("pipeline_name=None builds the face encoder only: there is no U-Net to put an IP-Adapter on")
        if self.ip_adapter is not None:
            self.unload_ip_adapter()
        unet = self.ldm.model.diffusion_model
        ad = path_or_obj
        if not isinstance(ad, IP.IPAdapter):
            cfg = dict(model_channels=unet.model_channels, num_res_blocks=unet.num_res_blocks, attention_resolutions=unet.attention_resolutions,
                       channel_mult=unet.channel_mult, num_heads=unet.num_heads, context_dim=unet._cross_attn_layers()[0].to_k.in_features)
            ad = IP.load_ip_adapter(ad, cfg)
        unet.check_ip_adapter(ad)                                # refuses widths or a layer count that do not match this U-Net
        enc = image_encoder
        if enc is not None and not isinstance(enc, vit.VisionTransformer):
            enc = vit.load_clip_vision(enc)
        if enc is not None and enc.feature_dim != ad.embed_dim:
            raise ValueError(f"the image encoder's features are {enc.feature_dim} wide, the adapter's image_proj reads {ad.embed_dim}")
        ad.fuse(self.ldm.model, lora_scale)
        self.__dict__["ip_adapter"], self.__dict__["ip_image_encoder"] = ad, enc
        return ad

    def unload_ip_adapter(self):
        ad = self.ip_adapter
        self.__dict__["ip_adapter"], self.__dict__["ip_image_encoder"] = None, None
        if ad is not None:
            ad.unfuse()
        if self.ldm is not None:
            self.ldm.model.diffusion_model.set_ip_adapter(None)

    def _check_ip(self, image, face_id, scale, start, end, rows):
        """The refusals of forward(ip_adapter_image= / ip_adapter_face_id=) (INTEGRATION.md "IP-Adapter"), all before any GPU work.  Returns
        ("images", [uint8 arrays]) or ("ids", fp32 [1 | rows, 512])."""
        ad = self.ip_adapter
        if ad is None:
            raise ValueError("ip_adapter_image / ip_adapter_face_id is given but no IP-Adapter is loaded (ip_adapter= at construction / load_ip_adapter)")
        if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not np.isfinite(scale):
            raise ValueError(f"ip_adapter_scale must be a finite number, got {scale!r}")
        ok = all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in (start, end))
        if not ok or not 0 <= start < end <= 1:
            raise ValueError(f"the IP-Adapter guidance window needs 0 <= ip_guidance_start < ip_guidance_end <= 1, got {start!r}, {end!r}")
        extractor = getattr(self.id2ada_prompt_encoder, "face_id_extractor", None)
        if face_id is not None:
            if ad.kind != "faceid":
                raise ValueError(f"ip_adapter_face_id is given but the loaded adapter is of kind {ad.kind!r}: it takes ip_adapter_image")
            if image is not None:
                raise ValueError("give ip_adapter_face_id or ip_adapter_image, not both")
            if not torch.is_tensor(face_id) or not face_id.is_floating_point() or face_id.dim() != 2 or face_id.shape[1] != ad.embed_dim:
                raise ValueError(f"ip_adapter_face_id must be a floating-point tensor [1 | {rows}, {ad.embed_dim}], got "
                                 f"{(face_id.dtype, tuple(face_id.shape)) if torch.is_tensor(face_id) else type(face_id).__name__}")
            if face_id.shape[0] not in (1, rows):
                raise ValueError(f"ip_adapter_face_id: 1 embedding (shared) or one per sampled row ({rows}) expected, got {face_id.shape[0]}")
            return "ids", face_id
        if ad.kind == "clip" and self.ip_image_encoder is None:
            raise ValueError("the loaded IP-Adapter is of kind 'clip' and needs an image encoder (ip_image_encoder= at construction / "
                             "load_ip_adapter(..., image_encoder=...))")
        if ad.kind == "faceid" and extractor is None:
            raise ValueError("the loaded adapter is of kind 'faceid': it takes ip_adapter_face_id, or ip_adapter_image with a face_id_extractor "
                             "at construction")
        items = list(image) if isinstance(image, (list, tuple)) else [image]
        flat = []
        for im in items:
            if torch.is_tensor(im) and im.dtype == torch.uint8 and im.dim() == 4 and im.shape[3] == 3:
                flat.extend(im.cpu().numpy())
            elif torch.is_tensor(im) and im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3:
                flat.append(im.cpu().numpy())
            elif isinstance(im, np.ndarray) and im.dtype == np.uint8 and im.ndim == 4 and im.shape[3] == 3:
                flat.extend(im)
            elif torch.is_tensor(im):
                raise ValueError(f"ip_adapter_image must be a PIL image, a path or uint8 [H, W, 3] / [B, H, W, 3], got {im.dtype} {tuple(im.shape)}")
            else:
                flat.append(im)
        if len(flat) not in (1, rows):
            raise ValueError(f"ip_adapter_image: 1 image (shared) or one per sampled row ({rows}) expected, got {len(flat)}")
        return "images", [load_rgb_u8(im) for im in flat]

    def _ip_tokens(self, what, value, rows):
        """(cond, uncond) image tokens fp16 [rows, T, context_dim], computed once per forward."""
        ad = self.ip_adapter.to(self.device)
        if what == "ids":
            embeds = nn.functional.normalize(value.float(), p=2, dim=-1)
        elif ad.kind == "faceid":
            faceless, embeds = self.id2ada_prompt_encoder.face_id_extractor.extract(value, skip_non_faces=False)
        else:
            enc = self.ip_image_encoder.to(self.device)
            embeds = torch.cat([enc.forward_u8(torch.from_numpy(np.ascontiguousarray(im))[None].to(self.device)) for im in value], 0)
        cond = ad.tokens(embeds)
        if cond.shape[0] == 1 and rows > 1:
            cond = cond.expand(rows, -1, -1).contiguous()
        return cond, ad.uncond_tokens(1).expand(rows, -1, -1).contiguous()

    def load_upscaler(self, path_or_net):
        """A Real-ESRGAN upscaler for ``forward(..., upscale=True)`` (adaface/esrgan.py; INTEGRATION.md "Upscaling (Real-ESRGAN)"): an
        ``Upscaler``, an ``RRDBNet``, or a local ``.pth`` file / state dict (loaded strictly by ``load_esrgan``).  Nothing is downloaded."""
        from . import esrgan
        up = path_or_net
        if not isinstance(up, esrgan.Upscaler):
            net = up if isinstance(up, esrgan.RRDBNet) else esrgan.load_esrgan(up)
            up = esrgan.Upscaler(net, device=self.device)
        self.__dict__["upscaler"] = up
        return up

    def unload_upscaler(self):
        self.__dict__["upscaler"] = None

    def load_face_restorer(self, path_or_net, detect_faces=None, **kwargs):
        """A GFPGAN face restorer for ``forward(..., restore_faces=True)`` (adaface/gfpgan.py; INTEGRATION.md "Face restoration (GFPGAN)"): a
        ``FaceRestorer``, a ``GFPGANv1Clean``, or a local ``.pth`` file / state dict (loaded strictly by ``load_gfpgan``).  The detector is
        ``detect_faces`` or, by default, the wrapper's ``face_detector``; ``kwargs`` go to ``FaceRestorer``.  Nothing is downloaded."""
        from . import gfpgan
        fr = path_or_net
        if not isinstance(fr, gfpgan.FaceRestorer):
            net = fr if isinstance(fr, gfpgan.GFPGANv1Clean) else gfpgan.load_gfpgan(fr)
            detect = detect_faces if detect_faces is not None else self.face_detector
            if detect is None:
                raise ValueError("a face restorer needs a detector: pass detect_faces, or build the wrapper with face_detector / face_id_extractor")
            fr = gfpgan.FaceRestorer(net, detect, device=self.device, **kwargs)
        self.__dict__["face_restorer"] = fr
        return fr

    def unload_face_restorer(self):
        self.__dict__["face_restorer"] = None

    def _check_restore(self):
        """The refusals of forward(restore_faces=True), ValueError before any GPU work."""
        if self.face_restorer is None:
            raise ValueError("restore_faces=True but no face restorer is loaded (face_restorer= at construction / load_face_restorer)")
        if self.vae is None:
            raise ValueError("restore_faces=True needs a vae: without one forward returns latents, which show no faces")

    def _restore(self, images_u8):
        """uint8 device images [B, H, W, 3] -> the same with every detected face restored (image by image: the detector takes one)."""
        return torch.stack([self.face_restorer.restore_u8(im) for im in images_u8])

    def _check_upscale(self, H, W):
        """The refusals of forward(upscale=True) for a result of H x W pixels, all ValueError before any GPU work."""
        if self.upscaler is None:
            raise ValueError("upscale=True but no upscaler is loaded (upscaler= at construction / load_upscaler)")
        if self.vae is None:
            raise ValueError("upscale=True needs a vae: without one forward returns latents, which are not upscaled")
        if H is not None:
            self.upscaler.check_size(int(H), int(W))

    def _check_video(self, noise, num_frames, out_image_count, hires_size):
        """The refusals of forward(num_frames=F) (INTEGRATION.md "Video (motion modules)"), all before any GPU work."""
        if self.motion_module is None:
            raise ValueError("num_frames is given but no motion module is loaded (motion_module_path / load_motion_module)")
        if self.pipeline_name != "text2img":
            raise ValueError(f"num_frames is given but the pipeline is {self.pipeline_name!r}: only pipeline_name='text2img' generates video")
        if hires_size is not None:
            raise ValueError("num_frames together with hires_size: two-pass high-resolution video is not built")
        if isinstance(num_frames, bool) or not isinstance(num_frames, int) or not 1 <= num_frames <= self.motion_module.max_len:
            raise ValueError(f"num_frames must be an integer from 1 to {self.motion_module.max_len} (the module's position table), got {num_frames!r}")
        if not torch.is_tensor(noise) or noise.dim() != 4 or noise.shape[0] != out_image_count * num_frames:
            raise ValueError(f"video noise must be [out_image_count * num_frames = {out_image_count * num_frames}, 4, h, w], video-major; got "
                             f"{tuple(noise.shape) if torch.is_tensor(noise) else type(noise).__name__}")

    def fuse_lcm_lora(self, path_or_state_dict, scale=1.0):
        """Fuse an SD-1.5 U-Net LoRA (a .safetensors / .bin / .pt file or a state dict in the kohya, diffusers or peft layout;
        adaface/sd_lora.py) into the U-Net weights: W' = W + scale * (alpha / r) * up @ down.  A LoRA fused earlier is unfused first.
        Raises RuntimeError while an AdaFace DoRA adapter merge is live.  Do not replay a graph captured before the fuse."""
        if self.ldm is None:
            raise RuntimeError("pipeline_name=None builds the face encoder only: there is no U-Net to fuse a LoRA into")
        sd_lora.check_no_live_merge(self.ldm.model)
        lora = sd_lora.read_unet_lora(path_or_state_dict, self.ldm.model)
        self.unfuse_lcm_lora()
        self._lcm_saved = sd_lora.fuse_unet_lora(self.ldm.model, lora, scale)
        self._lcm_lora = (lora, scale)

    def unfuse_lcm_lora(self):
        """Restore the U-Net weights saved by fuse_lcm_lora, bit-exactly (nothing to do when no LoRA is fused).  Raises RuntimeError
        while an AdaFace DoRA adapter merge is live."""
        if self.ldm is not None:
            sd_lora.check_no_live_merge(self.ldm.model)
        if self._lcm_saved:
            sd_lora.unfuse_unet_lora(self.ldm.model, self._lcm_saved)
        self._lcm_saved = {}
        self._lcm_lora = None

    def load_subj_basis_generator(self, adaface_ckpt_paths):
        """``embeddings_gs-N.pt`` as written by ``EmbeddingManager.save`` (pickled generator modules; the reference's class paths
        are mapped to the mirrors by adaface/ckpt.py), or a plain state dict of ``subj_basis_generator``."""
        from .ckpt import load_adaface_ckpt_file
        path = adaface_ckpt_paths[0] if isinstance(adaface_ckpt_paths, (list, tuple)) else adaface_ckpt_paths
        ck = load_adaface_ckpt_file(path.split(":")[0])
        if isinstance(ck, dict) and "string_to_subj_basis_generator_dict" in ck:
            self.id2ada_prompt_encoder.subject_string = self.subject_string
            return self.id2ada_prompt_encoder.load_adaface_ckpt(path)
        sd = ck.get("subj_basis_generator", ck)
        if not isinstance(sd, dict):
            sd = sd.state_dict()
        return self.id2ada_prompt_encoder.subj_basis_generator.load_state_dict(sd, strict=False)

    # ------------------------------------------------------------------ tokens (reference :414-489)
    def extend_tokenizer_and_text_encoder(self):
        if np.sum(self.encoders_num_id_vecs) < 1:
            raise ValueError(f"encoders_num_id_vecs has to be larger or equal to 1, but is {self.encoders_num_id_vecs}")
        self.all_placeholder_tokens, self.placeholder_tokens_strs, self.encoder_placeholder_tokens = [], [], []
        for i in range(len(self.adaface_encoder_types)):
            toks = [f"{self.subject_string}_{i}_{j}" for j in range(self.encoders_num_id_vecs[i])]
            self.all_placeholder_tokens.extend(toks)
            self.encoder_placeholder_tokens.append(toks)
            self.placeholder_tokens_strs.append(" ".join(toks))
        self.all_placeholder_tokens_str = " ".join(self.placeholder_tokens_strs)
        self.updated_tokens_str = self.all_placeholder_tokens_str
        self.all_encoders_updated_token_strs = list(self.placeholder_tokens_strs)
        self.all_null_placeholder_tokens_str = " ".join([", "] * len(self.all_placeholder_tokens))
        n = self.tokenizer.add_tokens(self.all_placeholder_tokens)
        if n != np.sum(self.encoders_num_id_vecs):
            raise ValueError(f"The tokenizer already contains some of the tokens {self.all_placeholder_tokens_str}. Please pass a different"
                             " `subject_string` that is not already in the tokenizer.")
        self.placeholder_token_ids = self.tokenizer.convert_tokens_to_ids(self.all_placeholder_tokens)
        emb = self.text_encoder.text_model.embeddings.token_embedding                  # resize_token_embeddings(len(tokenizer))
        if emb.num_embeddings < len(self.tokenizer):
            new = nn.Embedding(len(self.tokenizer), emb.embedding_dim).to(device=emb.weight.device, dtype=emb.weight.dtype)
            with torch.no_grad():
                new.weight[:emb.num_embeddings] = emb.weight
                new.weight[emb.num_embeddings:] = emb.weight.mean(dim=0, keepdim=True)
            new.weight.requires_grad_(emb.weight.requires_grad)
            self.text_encoder.text_model.embeddings.token_embedding = new

    def update_text_encoder_subj_embeddings(self, subj_embs, lens_subj_emb_segments):
        token_embeds = self.text_encoder.text_model.embeddings.token_embedding.weight.data
        all_tokens, all_strs, idx = [], [], 0
        with torch.no_grad():
            for i, encoder_type in enumerate(self.adaface_encoder_types):
                if (self.enabled_encoders is not None) and (encoder_type not in self.enabled_encoders):
                    idx += lens_subj_emb_segments[i]
                    continue
                toks = []
                for j in range(lens_subj_emb_segments[i]):
                    tok = f"{self.subject_string}_{i}_{j}"
                    token_embeds[self.tokenizer.convert_tokens_to_ids(tok)] = subj_embs[idx].to(token_embeds.dtype)
                    toks.append(tok)
                    idx += 1
                all_tokens.extend(toks)
                all_strs.append(" ".join(toks))
        self.updated_tokens_str = " ".join(all_strs)
        self.all_encoders_updated_token_strs = all_strs

    def update_prompt(self, prompt, placeholder_tokens_pos="append", repeat_prompt_for_each_encoder=True, use_null_placeholders=False):
        if prompt is None:
            prompt = ""
        if use_null_placeholders:
            all_placeholder_tokens_str = self.all_null_placeholder_tokens_str
            if not re.search(r"\b(man|woman|person|child|girl|boy)\b", prompt.lower()):
                all_placeholder_tokens_str = "person " + all_placeholder_tokens_str
            repeat_prompt_for_each_encoder = False
        else:
            all_placeholder_tokens_str = self.updated_tokens_str
        prompt = re.sub(r"\b(a|an|the)\s+" + self.subject_string + r"\b,?", "", prompt)
        prompt = re.sub(r"\b" + self.subject_string + r"\b,?", "", prompt)
        if placeholder_tokens_pos not in ("prepend", "append"):
            raise ValueError(f"placeholder_tokens_pos {placeholder_tokens_pos!r}")
        join = (lambda toks: toks + " " + prompt) if placeholder_tokens_pos == "prepend" else (lambda toks: prompt + " " + toks)
        if repeat_prompt_for_each_encoder:
            return ", ".join(join(s) for s in self.all_encoders_updated_token_strs)
        return join(all_placeholder_tokens_str)

    # ------------------------------------------------------------------ embeddings (reference :541-569, 671-727)
    def prepare_adaface_embeddings(self, image_paths, face_id_embs=None, avg_at_stage="id_emb", perturb_at_stage=None, perturb_std=0,
                                   update_text_encoder=True):
        if face_id_embs is not None and face_id_embs.shape[0] > 1 and avg_at_stage == "id_emb":
            # pre-extracted IDs of several images of the subject: the 'id_emb' averaging of the reference lives in its image -> ID
            # extraction (insightface, absent here), so it is applied to the IDs brought in instead
            face_id_embs = self.id2ada_prompt_encoder.average_id_embs(face_id_embs)
        embs, img_prompt_embs, lens = self.id2ada_prompt_encoder.generate_adaface_embeddings(
            image_paths, face_id_embs=face_id_embs, img_prompt_embs=None, avg_at_stage=avg_at_stage, perturb_at_stage=perturb_at_stage,
            perturb_std=perturb_std, enable_static_img_suffix_embs=self.enable_static_img_suffix_embs)
        if embs is None:
            return None
        self.img_prompt_embs = img_prompt_embs
        if embs.ndim == 4:
            embs = embs.squeeze(0).squeeze(0)
        elif embs.ndim == 3:
            embs = embs.squeeze(0)
        if update_text_encoder:
            self.update_text_encoder_subj_embeddings(embs, lens)
        return embs

    @torch.no_grad()
    def _encode(self, texts, device):
        ids = self.tokenizer(texts, padding="max_length", max_length=self.max_prompt_length, truncation=True, return_tensors="pt").input_ids
        return self.text_encoder(input_ids=ids.to(device))[0]

    def encode_prompt(self, prompt, negative_prompt=None, placeholder_tokens_pos="append", ablate_prompt_only_placeholders=False,
                      ablate_prompt_no_placeholders=False, ablate_prompt_embed_type="ada", nonmix_prompt_emb_weight=0,
                      repeat_prompt_for_each_encoder=True, device=None, verbose=False):
        if negative_prompt is None:
            negative_prompt = self.negative_prompt
        device = device or self.device
        if ablate_prompt_embed_type != "ada" or nonmix_prompt_emb_weight > 0:
            raise NotImplementedError("image-prompt mixing ablations (mix_ada_embs_with_other_embs) are not built")
        if ablate_prompt_only_placeholders:
            prompt = self.updated_tokens_str
        else:
            prompt = self.update_prompt(prompt, placeholder_tokens_pos=placeholder_tokens_pos,
                                        repeat_prompt_for_each_encoder=repeat_prompt_for_each_encoder,
                                        use_null_placeholders=ablate_prompt_no_placeholders)
        if verbose:
            print(f"Subject prompt:\n{prompt}")
        self.text_encoder.to(device)
        return self._encode([prompt], device), self._encode([negative_prompt], device), None, None

    # ------------------------------------------------------------------ generation (reference :730-809)
    @torch.no_grad()
    def forward(self, noise, prompt, prompt_embeds=None, negative_prompt=None, placeholder_tokens_pos="append", guidance_scale=6.0,
                out_image_count=4, ref_img_strength=0.8, generator=None, ablate_prompt_only_placeholders=False,
                ablate_prompt_no_placeholders=False, ablate_prompt_embed_type="ada", nonmix_prompt_emb_weight=0,
                repeat_prompt_for_each_encoder=True, verbose=False, mask_image=None, hires_size=None, hires_strength=0.7,
                hires_steps=None, hires_upscaler="bilinear", crop_padding=None, face_index=None, face_mask_expand=1.3,
                face_mask_feather=0.25, work_size=None, num_frames=None, upscale=False, restore_faces=False, control_image=None,
                control_scale=1.0, control_guidance_start=0.0, control_guidance_end=1.0, ip_adapter_image=None, ip_adapter_face_id=None,
                ip_adapter_scale=1.0, ip_guidance_start=0.0, ip_guidance_end=1.0, region_masks=None, region_prompts=None,
                region_prompt_embeds=None, region_base_weight=0.2):
        if self.ldm is None:
            raise RuntimeError("pipeline_name=None builds the face encoder only")
        if upscale:
            self._check_upscale(None, None)
        if restore_faces:
            self._check_restore()
        if num_frames is not None:
            self._check_video(noise, num_frames, out_image_count, hires_size)
            videos = out_image_count
            out_image_count = videos * num_frames          # the batch is video-major: row v * F + f, the prompt repeated per frame
        repaint = self._check_repaint(noise, mask_image, crop_padding, face_index, face_mask_expand, face_mask_feather, work_size)
        control = None
        if control_image is not None:
            control = (self._check_control(control_image, control_scale, control_guidance_start, control_guidance_end, out_image_count,
                                           hires_size, repaint), float(control_scale), control_guidance_start, control_guidance_end)
        ip_in = None
        if ip_adapter_image is not None or ip_adapter_face_id is not None:
            ip_in = self._check_ip(ip_adapter_image, ip_adapter_face_id, ip_adapter_scale, ip_guidance_start, ip_guidance_end, out_image_count)
        region_masks_u8 = None
        if region_masks is not None or region_prompts is not None or region_prompt_embeds is not None:
            region_masks_u8 = self._check_regions(region_masks, region_prompts, region_prompt_embeds, region_base_weight, num_frames, hires_size,
                                                  crop_padding)
            if repaint is not None:
                raise ValueError("regional prompts are not built with repainting a photo (mask_image='face' or crop_padding)")
        if hires_size is not None:
            hires_hw, hires_steps = self._check_hires(hires_size, hires_strength, hires_steps, hires_upscaler)
        if upscale and self.pipeline_name == "text2img":
            if hires_size is not None:
                self._check_upscale(hires_hw[0] * 8, hires_hw[1] * 8)
            elif torch.is_tensor(noise) and noise.dim() == 4:
                self._check_upscale(noise.shape[2] * 8, noise.shape[3] * 8)
        inpaint = self.pipeline_name == "inpaint"
        if inpaint and mask_image is None:
            raise ValueError("the inpaint pipeline needs mask_image (white = repaint)")
        if not inpaint and mask_image is not None:
            raise ValueError(f"mask_image is given but the pipeline is {self.pipeline_name!r}: only pipeline_name='inpaint' takes a mask")
        if self.pipeline_name in ("img2img", "inpaint"):
            if self.vae is None or not hasattr(self.vae, "encode_q_sample"):
                raise ValueError(f"the {self.pipeline_name} pipeline encodes its input images: it needs an AutoencoderKL (encoder + "
                                 f"decoder) as vae, got {type(self.vae).__name__ if self.vae is not None else None}")
            if repaint is not None:
                self._sampler().img2img_steps(self.num_inference_steps, ref_img_strength)    # (before the detector runs)
                repaint = self._repaint_plan(noise, mask_image, out_image_count, repaint, upscale)
                images_u8 = None
            else:
                images_u8 = img2img_images_u8(noise, out_image_count)
            if images_u8 is not None and max(images_u8.shape[1:3]) > MAX_IMAGE_SIDE:
                raise ValueError(f"{self.pipeline_name} input images may be at most {MAX_IMAGE_SIDE} pixels on a side (the VAE's limit), got "
                                 f"{images_u8.shape[2]} x {images_u8.shape[1]}")
            if upscale and images_u8 is not None:
                self._check_upscale(images_u8.shape[1], images_u8.shape[2])
            if inpaint and repaint is None:
                masks = inpaint_masks(mask_image, out_image_count, (images_u8.shape[2], images_u8.shape[1]))
            self._sampler().img2img_steps(self.num_inference_steps, ref_img_strength)    # refuse a bad strength before any work
            if control is not None:
                self._check_control_size(control[0], (images_u8.shape[1] // 8, images_u8.shape[2] // 8))
            if region_masks_u8 is not None:
                self._check_region_size(region_masks_u8, tuple(images_u8.shape[1:3]))
        elif self.vae is not None and torch.is_tensor(noise) and noise.dim() == 4 and max(noise.shape[2:]) * 8 > MAX_IMAGE_SIDE:
            raise ValueError(f"text2img latents may be at most {MAX_IMAGE_SIDE // 8} on a side ({MAX_IMAGE_SIDE} pixels, the VAE's limit), got "
                             f"noise of shape {tuple(noise.shape)}")
        if control is not None and self.pipeline_name == "text2img":
            if not torch.is_tensor(noise) or noise.dim() != 4:
                raise ValueError("control_image needs noise [rows, 4, h, w] to take the latent size from")
            self._check_control_size(control[0], tuple(noise.shape[2:]))
        if region_masks_u8 is not None and self.pipeline_name == "text2img":
            if not torch.is_tensor(noise) or noise.dim() != 4:
                raise ValueError("region_masks need noise [rows, 4, h, w] to take the image size from")
            self._check_region_size(region_masks_u8, (noise.shape[2] * 8, noise.shape[3] * 8))
        if prompt_embeds is None:
            pe, ne, _, _ = self.encode_prompt(prompt, negative_prompt, placeholder_tokens_pos=placeholder_tokens_pos,
                                              ablate_prompt_only_placeholders=ablate_prompt_only_placeholders,
                                              ablate_prompt_no_placeholders=ablate_prompt_no_placeholders,
                                              ablate_prompt_embed_type=ablate_prompt_embed_type,
                                              nonmix_prompt_emb_weight=nonmix_prompt_emb_weight,
                                              repeat_prompt_for_each_encoder=repeat_prompt_for_each_encoder, device=self.device, verbose=verbose)
        elif len(prompt_embeds) in (2, 4):
            pe, ne = prompt_embeds[0], prompt_embeds[1]
        else:
            raise ValueError("prompt_embeds must be a 2- or 4-tuple")
        pe = pe.repeat(out_image_count, 1, 1)
        ne = None if ne is None else ne.repeat(out_image_count, 1, 1)
        self.ldm.to(self.device)
        sampler = self._sampler()
        cond = (pe, [prompt or ""] * out_image_count, {})
        uncond = None if ne is None else (ne, [negative_prompt or self.negative_prompt] * out_image_count, {})
        ip = None
        if ip_in is not None:
            ip = self._ip_tokens(ip_in[0], ip_in[1], out_image_count) + (float(ip_adapter_scale), ip_guidance_start, ip_guidance_end)
        regions = None
        if region_masks_u8 is not None:
            regions = self._region_state(region_masks_u8, region_prompts, region_prompt_embeds, region_base_weight, pe.to(self.device),
                                         None if ne is None else ne.to(self.device),
                                         dict(placeholder_tokens_pos=placeholder_tokens_pos, repeat_prompt_for_each_encoder=repeat_prompt_for_each_encoder))
        if self.pipeline_name == "img2img":
            n_run, t_first = sampler.img2img_steps(self.num_inference_steps, ref_img_strength)
            x_t = self.ldm.img2img_latents(images_u8.to(self.device), out_image_count, t_first, generator=generator,
                                           first_stage_model=self.vae)
            latents, _ = self._sample_controlled(control, n_run, lambda **cb: sampler.sample_img2img(
                self.num_inference_steps, ref_img_strength, out_image_count, x_t, cond, guidance_scale=guidance_scale,
                unconditional_conditioning=uncond, generator=generator, **cb), ip, regions)
            return self._to_pil(latents, upscale, restore_faces)
        if inpaint:
            n_run, t_first = sampler.img2img_steps(self.num_inference_steps, ref_img_strength)
            if repaint is not None:
                photo = torch.from_numpy(repaint["photo"]).to(self.device)
                if repaint["ellipses"] is not None:
                    alpha = ops.face_alpha_mask(torch.from_numpy(repaint["ellipses"]).to(self.device), photo.shape[:2], repaint["feather"])
                else:
                    alpha = torch.from_numpy(repaint["hard_mask"]).to(self.device)
                images_u8, masks = ops.crop_resize_u8(photo, alpha, repaint["rect"], repaint["work_hw"], 1.0 / 255.0)
            x_start, z, n_fwd = self.ldm.inpaint_latents(images_u8.to(self.device), out_image_count, t_first, generator=generator,
                                                         first_stage_model=self.vae, from_noise=ref_img_strength == 1)
            latents, _ = self._sample_controlled(control, n_run, lambda **cb: sampler.sample_inpaint(
                self.num_inference_steps, ref_img_strength, out_image_count, x_start, z, n_fwd, masks.to(self.device), cond,
                guidance_scale=guidance_scale, unconditional_conditioning=uncond, generator=generator, **cb), ip, regions)
            if repaint is not None:
                return self._paste_back(latents, photo, alpha, repaint["rect"], upscale, restore_faces)
            return self._to_pil(latents, upscale, restore_faces)
        noise = noise.to(device=self.device, dtype=torch.float32)
        unet = self.ldm.model.diffusion_model
        if num_frames is not None:
            self.motion_module.to(self.device)
            unet.set_motion(self.motion_module, num_frames)           # around the sampling call only
        try:
            n_run = len(sampler.timesteps(self.num_inference_steps)) if control is not None or ip is not None else None
            latents, _ = self._sample_controlled(control, n_run, lambda **cb: sampler.sample(
                self.num_inference_steps, out_image_count, tuple(noise.shape[1:]), conditioning=cond, x_T=noise, verbose=False,
                guidance_scale=guidance_scale, unconditional_conditioning=uncond, generator=generator, **cb), ip, regions)
        finally:
            if num_frames is not None:
                unet.set_motion(None)
        if hires_size is not None:
            n_run2, t_first = sampler.img2img_steps(hires_steps, hires_strength)
            x_t = self.ldm.hires_latents(latents, hires_hw, t_first, generator, hires_upscaler)
            latents, _ = self._sample_controlled(None, n_run2, lambda **cb: sampler.sample_img2img(
                hires_steps, hires_strength, out_image_count, x_t, cond, guidance_scale=guidance_scale, unconditional_conditioning=uncond,
                generator=generator, **cb), ip)
        if self.vae is None:
            return latents
        if num_frames is not None:
            frames = self._to_pil(latents, upscale, restore_faces)
            return [frames[v * num_frames:(v + 1) * num_frames] for v in range(videos)]
        return self._to_pil(latents, upscale, restore_faces)

    def _check_hires(self, hires_size, hires_strength, hires_steps, hires_upscaler):
        """The refusals of high-resolution text2img (INTEGRATION.md "High-resolution text2img"), all before any GPU work.  Returns
        the second pass's latent (H, W) and its step count."""
        if self.pipeline_name != "text2img":
            raise ValueError(f"hires_size is given but the pipeline is {self.pipeline_name!r}: only pipeline_name='text2img' runs two passes")
        try:
            W, H = (int(s) for s in hires_size)
        except (TypeError, ValueError):
            raise ValueError(f"hires_size must be (W, H) in pixels, got {hires_size!r}") from None
        if W % 64 or H % 64 or not (64 <= W <= MAX_IMAGE_SIDE and 64 <= H <= MAX_IMAGE_SIDE):
            raise ValueError(f"hires_size sides must be multiples of 64 from 64 to {MAX_IMAGE_SIDE} pixels, got {W} x {H}")
        if hires_upscaler not in ops.RESIZE_MODES:
            raise ValueError(f"hires_upscaler must be one of {sorted(ops.RESIZE_MODES)}, got {hires_upscaler!r}")
        steps = self.num_inference_steps if hires_steps is None else hires_steps
        if not isinstance(steps, int) or not 1 <= steps <= self.ldm.num_timesteps:
            raise ValueError(f"hires_steps must be an integer from 1 to {self.ldm.num_timesteps}, got {hires_steps!r}")
        self._sampler().img2img_steps(steps, hires_strength)        # a bad strength, or more steps than the sampler takes
        return (H // 8, W // 8), steps

    def _check_repaint(self, photo, mask_image, crop_padding, face_index, face_mask_expand, face_mask_feather, work_size):
        """The refusals of the photo-level inpaint path (INTEGRATION.md "Repainting faces in a photo"), all before any GPU work.  Returns
        None for the plain paths (a PIL mask without crop_padding included), else the checked settings."""
        face = isinstance(mask_image, str)
        if face and mask_image != "face":
            raise ValueError(f"mask_image as a string must be 'face', got {mask_image!r}")
        if self.pipeline_name != "inpaint":
            for name, v in (("crop_padding", crop_padding), ("face_index", face_index), ("work_size", work_size)):
                if v is not None:
                    raise ValueError(f"{name} is given but the pipeline is {self.pipeline_name!r}: only pipeline_name='inpaint' repaints a "
                                     "region of a photo")
            return None                             # (a mask_image on another pipeline is refused by forward itself)
        if face and self.face_detector is None:
            raise FaceDetectorMissing("mask_image='face' needs a face detector: pass face_detector (e.g. a RetinaFaceDetector) or a "
                                      "face_id_extractor at construction")
        if face_index is not None and not face:
            raise ValueError("face_index selects among detected faces: it needs mask_image='face'")
        if face_index is not None and (isinstance(face_index, bool) or not isinstance(face_index, (int, np.integer)) or face_index < 0):
            raise ValueError(f"face_index must be a non-negative integer, got {face_index!r}")
        if crop_padding is not None and not (isinstance(crop_padding, (int, float)) and 0 <= crop_padding < float("inf")):
            raise ValueError(f"crop_padding must be a finite number >= 0 (or None), got {crop_padding!r}")
        if not (isinstance(face_mask_expand, (int, float)) and 0 < face_mask_expand < float("inf")):
            raise ValueError(f"face_mask_expand must be a finite positive number, got {face_mask_expand!r}")
        if not (isinstance(face_mask_feather, (int, float)) and 0 <= face_mask_feather < float("inf")):
            raise ValueError(f"face_mask_feather must be a finite number >= 0, got {face_mask_feather!r}")
        if work_size is not None and crop_padding is None:
            raise ValueError("work_size is the size the crop is resampled to: it needs crop_padding (without it the photo runs at its own size)")
        work_hw = None
        if crop_padding is not None:
            work_hw = face_repaint.check_work_size((512, 512) if work_size is None else work_size, MAX_IMAGE_SIDE)
        if not face and crop_padding is None:
            return None
        if isinstance(photo, (list, tuple)):
            if len(photo) != 1:
                raise ValueError(f"repainting a photo (mask_image='face' or crop_padding) takes one photo, got {len(photo)}")
            photo = photo[0]
        if not face and isinstance(mask_image, (list, tuple)):
            if len(mask_image) != 1:
                raise ValueError(f"crop_padding takes one mask image, got {len(mask_image)}")
        return dict(face=face, crop_padding=crop_padding, face_index=face_index, expand=float(face_mask_expand),
                    feather=float(face_mask_feather), work_hw=work_hw)

    def _repaint_plan(self, photo, mask_image, out_image_count, cfg, upscale=False):
        """Host preparation of the photo-level path: the photo's bytes, the ellipses (or the hard mask), the rectangle and the working
        size.  The detector is the only GPU work in here."""
        from PIL import Image
        if isinstance(photo, (list, tuple)):
            photo = photo[0]
        rgb = load_rgb_u8(photo)
        if cfg["crop_padding"] is None:             # the whole photo at its own size, under img2img's size rules
            rgb = np.ascontiguousarray(img2img_images_u8(Image.fromarray(rgb), out_image_count)[0].numpy())
            if max(rgb.shape[:2]) > MAX_IMAGE_SIDE:
                raise ValueError(f"without crop_padding the whole photo is repainted: it may be at most {MAX_IMAGE_SIDE} pixels on a side "
                                 f"(the VAE's limit), got {rgb.shape[1]} x {rgb.shape[0]}; pass crop_padding to repaint a region")
        H, W = rgb.shape[:2]
        if upscale:                                 # the photo comes back upscaled: refuse its size before the detector runs
            self._check_upscale(H, W)
        if H * W * 3 >= 1 << 31:
            raise ValueError(f"the photo needs 2^31 bytes or more ({W} x {H}): the kernels use 32-bit offsets")
        plan = dict(photo=rgb, ellipses=None, hard_mask=None, feather=cfg["feather"])
        if cfg["face"]:
            plan["ellipses"] = face_repaint.face_ellipses(self.face_detector(rgb), cfg["face_index"], cfg["expand"])
            boxes = face_repaint.ellipse_boxes(plan["ellipses"])
        else:
            m = mask_image[0] if isinstance(mask_image, (list, tuple)) else mask_image
            if not isinstance(m, Image.Image):
                raise ValueError(f"inpainting mask images must be PIL images (or the string 'face'), got {type(m).__name__}")
            m = m.convert("L")
            if m.size != (W, H):
                m = m.resize((W, H), resample=Image.LANCZOS)
            hard = np.asarray(m, dtype=np.uint8) >= 128
            boxes = face_repaint.mask_bbox(hard)
            plan["hard_mask"] = hard.astype(np.float32)
        if cfg["crop_padding"] is None:
            plan["rect"], plan["work_hw"] = (0, 0, W, H), (H, W)
        else:
            plan["work_hw"] = cfg["work_hw"]
            plan["rect"] = face_repaint.crop_region(boxes, (H, W), cfg["work_hw"], cfg["crop_padding"])
        return plan

    def _paste_back(self, latents, photo, alpha, rect, upscale=False, restore_faces=False):
        """Decode, then one ``ops.paste_back_u8`` launch and one device-to-host copy (per slice of photos that stays below 2^31 bytes); under
        ``restore_faces`` and ``upscale`` the pasted photos go through the face restorer and then the upscaler on the device in between."""
        from PIL import Image
        decoded = self._decode(latents).float().contiguous()
        per = max(1, (2 ** 31 - 1) // photo.numel())
        out = []
        for i in range(0, decoded.shape[0], per):
            part = ops.paste_back_u8(decoded[i:i + per], photo, alpha, rect)
            if restore_faces:
                part = self._restore(part)
            out.append((self.upscaler.upscale_u8(part) if upscale else part).cpu().numpy())
        return [Image.fromarray(im) for part in out for im in part]

    def _sampler(self):
        return LCMSampler(self.ldm) if self.use_lcm else SCHEDULERS[self.default_scheduler_name](self.ldm)

    def _decode(self, latents):
        # decode in slices of images that keep the widest activation (256 channels at full resolution) below 2^31 elements, the bound of the
        # kernels' 32-bit offsets: 8 images at 1024 x 1024, 32 at 512 x 512 -- one slice for every batch the pipelines run by default
        per = max(1, (2 ** 31 - 1) // (latents.shape[2] * latents.shape[3] * 64 * 256))
        return torch.cat([self.vae.decode(latents[i:i + per] / 0.18215) for i in range(0, latents.shape[0], per)])

    def _to_pil(self, latents, upscale=False, restore_faces=False):
        images = self._decode(latents)
        images = ((images.float() / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1)
        if restore_faces:                           # before the upscaler: it sharpens what the restorer leaves, artefacts included
            images = self._restore(images.contiguous())
        if upscale:                                 # on the device, in slices of images (Upscaler.upscale_u8): no host round trip
            images = self.upscaler.upscale_u8(images.contiguous())
        images = images.cpu().numpy()
        from PIL import Image
        return [Image.fromarray(im) for im in images]
