"""The reference's scoring classes (``evaluation/clip_eval.py``: ``CLIPEvaluator``, ``ImageDirEvaluator``; ``evaluation/eval_utils.py``: the
DINO ``ViTEvaluator`` and ``compare_face_folders``), on the encoders of ``evaluation/vit.py`` and ``adaface/face_align.FaceIDExtractor``.
Names and call shapes follow the reference; the reference tree is not available here, so the contract is restated (INTEGRATION.md "Scoring
images").  Three numbers come out: CLIP-I (image-to-image), CLIP-T (text-to-image) / DINO (image-to-image) and the face similarity.

Images are accepted as paths, PIL images, uint8 arrays, uint8 tensors [B, H, W, 3] (or [H, W, 3]) and -- the reference's input -- float
tensors [B, 3, H, W] in [-1, 1].  Everything becomes uint8 on the device and goes through ``af_vit_patch_rows``; a float tensor is therefore
quantised first, ``rint(255 clamp(x / 2 + 1/2, 0, 1))``, where the reference resamples the floats (a deviation of at most half a grey level per
input pixel).  Images of different sizes are grouped by size, one preprocess launch per group of at most ``max_batch``; features come back in
input order."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from ..adaface.face_align import load_rgb_u8
from . import vit

IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".webp")


def float_images_to_u8(x):
    """float [B, 3, H, W] (or [3, H, W]) in [-1, 1] -> uint8 [B, H, W, 3]: rint(255 clamp(x / 2 + 1/2, 0, 1)), ties to even."""
    if x.dim() == 3:
        x = x[None]
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"a float image tensor must be [B, 3, H, W] in [-1, 1], got {tuple(x.shape)}")
    return torch.round(255.0 * (x.float() / 2 + 0.5).clamp(0, 1)).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def images_to_u8_list(images):
    """Any accepted form -> a list of uint8 tensors [H, W, 3], one per image, in input order (on whatever device they arrived on)."""
    if torch.is_tensor(images):
        if images.is_floating_point():
            return list(float_images_to_u8(images))
        if images.dtype != torch.uint8 or images.dim() not in (3, 4) or images.shape[-1] != 3:
            raise ValueError(f"an image tensor must be uint8 [B, H, W, 3] or float [B, 3, H, W], got {images.dtype} {tuple(images.shape)}")
        return list(images if images.dim() == 4 else images[None])
    if isinstance(images, (str, bytes, np.ndarray)) or hasattr(images, "__fspath__") or not hasattr(images, "__iter__"):
        images = [images]
    out = []
    for im in images:
        if torch.is_tensor(im):
            out.extend(images_to_u8_list(im))
        else:
            out.append(torch.from_numpy(load_rgb_u8(im)))
    return out


def size_groups(shapes, max_batch):
    """Indices of equal (H, W), in order of first appearance, cut into runs of at most max_batch."""
    if max_batch < 1:
        raise ValueError(f"max_batch must be at least 1, got {max_batch}")
    by = {}
    for i, s in enumerate(shapes):
        by.setdefault(tuple(s), []).append(i)
    return [idx[j:j + max_batch] for idx in by.values() for j in range(0, len(idx), max_batch)]


def encode_grouped(images, encode_u8, device, max_batch=64):
    """features [N, D] fp32 in input order from ``encode_u8(uint8 [b, H, W, 3] on device) -> [b, D]``, one call per size group."""
    ims = images_to_u8_list(images)
    if not ims:
        raise ValueError("no images to encode")
    out = [None] * len(ims)
    for idx in size_groups([im.shape[:2] for im in ims], max_batch):
        batch = torch.stack([ims[i].to(device) for i in idx]).contiguous()
        feats = encode_u8(batch).float()
        for j, i in enumerate(idx):
            out[i] = feats[j]
    return torch.stack(out)


def list_image_files(folder):
    return sorted(os.path.join(folder, f) for f in os.listdir(folder) if f.lower().endswith(IMAGE_EXTENSIONS))


class CLIPEvaluator:
    """``clip_model``: a checkpoint file or state dict (``vit.load_clip``), or the pair ``(vision, text)``: anything with
    ``forward_u8(uint8 images) -> features`` and ``encode(token ids) -> features``.  ``tokenizer``: a transformers-protocol CLIP tokenizer;
    the fallback is the deterministic ``WordTokenizer`` stand-in (there are no vocabulary files offline), whose scores mean nothing against
    real CLIP weights."""
    context_length = 77

    def __init__(self, device, clip_model="ViT-B/32", tokenizer=None, max_batch=64):
        self.device = torch.device(device)
        if isinstance(clip_model, (tuple, list)):
            vision, text = clip_model
        elif isinstance(clip_model, dict) or os.path.exists(str(clip_model)):
            vision, text = vit.load_clip(clip_model)
        else:
            raise ValueError(f"CLIPEvaluator: clip_model must be a local checkpoint file, a state dict or a (vision, text) pair; {clip_model!r} is "
                             "not a file (nothing is downloaded)")
        self.vision = vision.to(self.device).eval() if isinstance(vision, torch.nn.Module) else vision
        self.text = text.to(self.device).eval() if isinstance(text, torch.nn.Module) else text
        if tokenizer is None:
            from ..adaface.adaface_wrapper import WordTokenizer
            tokenizer = WordTokenizer()
        self.tokenizer = tokenizer
        self.max_batch = max_batch

    def tokenize(self, strings):
        enc = self.tokenizer([strings] if isinstance(strings, str) else list(strings), padding="max_length", max_length=self.context_length,
                             truncation=True, return_tensors="pt")
        return enc["input_ids"].to(self.device)

    @torch.no_grad()
    def encode_text(self, tokens):
        return self.text.encode(tokens).float()

    @torch.no_grad()
    def encode_images(self, images):
        return encode_grouped(images, self.vision.forward_u8, self.device, self.max_batch)

    def get_text_features(self, text, norm=True):
        f = self.encode_text(self.tokenize(text))
        return F.normalize(f, dim=-1) if norm else f

    def get_image_features(self, images, norm=True):
        f = self.encode_images(images)
        return F.normalize(f, dim=-1) if norm else f

    def img_to_img_similarity(self, src_images, generated_images):
        return float((self.get_image_features(src_images) @ self.get_image_features(generated_images).T).mean())

    def txt_to_img_similarity(self, text, generated_images):
        return float((self.get_text_features(text) @ self.get_image_features(generated_images).T).mean())


class ImageDirEvaluator(CLIPEvaluator):
    def evaluate(self, gen_samples, src_images, target_text):
        """-> (CLIP-I, CLIP-T).  Placeholder stars are stripped from the prompt, as in the reference."""
        sim_img = self.img_to_img_similarity(src_images, gen_samples)
        sim_text = self.txt_to_img_similarity(target_text.replace("*", ""), gen_samples)
        return sim_img, sim_text


class ViTEvaluator:
    """DINO image-to-image similarity.  ``dino_model``: a checkpoint file or state dict (``vit.load_dino``) or anything with ``forward_u8``."""

    def __init__(self, device, dino_model="dino_vits16", max_batch=64):
        self.device = torch.device(device)
        if isinstance(dino_model, dict) or (isinstance(dino_model, (str, os.PathLike)) and os.path.exists(str(dino_model))):
            dino_model = vit.load_dino(dino_model)
        elif isinstance(dino_model, (str, os.PathLike)):
            raise ValueError(f"ViTEvaluator: dino_model must be a local checkpoint file, a state dict or a model; {dino_model!r} is not a file "
                             "(nothing is downloaded)")
        self.model = dino_model.to(self.device).eval() if isinstance(dino_model, torch.nn.Module) else dino_model
        self.max_batch = max_batch

    @torch.no_grad()
    def get_image_features(self, images, norm=True):
        f = encode_grouped(images, self.model.forward_u8, self.device, self.max_batch)
        return F.normalize(f, dim=-1) if norm else f

    def img_to_img_similarity(self, src_images, generated_images):
        return float((self.get_image_features(src_images) @ self.get_image_features(generated_images).T).mean())


class FaceSimilarityEvaluator:
    """Cosine of face IDs between subject and generated images, on ``FaceIDExtractor.extract`` (unit-norm IDs of the largest face per image)."""

    def __init__(self, face_id_extractor):
        self.extractor = face_id_extractor

    def compare(self, src_images, gen_images):
        """-> (mean pairwise cosine, (faceless count of src, faceless count of gen)); 0.0 when either side shows no face."""
        n1, e1 = self.extractor.extract(_as_image_list(src_images))
        n2, e2 = self.extractor.extract(_as_image_list(gen_images))
        if e1 is None or e2 is None:
            return 0.0, (n1, n2)
        return float((e1.float() @ e2.float().T).mean()), (n1, n2)


def _as_image_list(images):
    """What ``FaceIDExtractor.extract`` iterates over: paths, PIL images or uint8 arrays."""
    if torch.is_tensor(images):
        return [im.cpu().numpy() for im in images_to_u8_list(images)]
    return [images] if isinstance(images, (str, bytes, np.ndarray)) or hasattr(images, "__fspath__") else list(images)


def compare_face_folders(path1, path2, face_id_extractor):
    """The reference's function over two folders of image files -> (similarity, (faceless in path1, faceless in path2))."""
    return FaceSimilarityEvaluator(face_id_extractor).compare(list_image_files(path1), list_image_files(path2))
