"""From photos of a person to the 512-d face IDs the Arc2Face / AdaFace encoders start from: what the reference gets from insightface's
``FaceAnalysis`` (``face_id_to_ada_prompt.py:249-350``, ``extract_init_id_embeds_from_images``), restated from insightface's own
``face_align.norm_crop`` + ``ArcFaceONNX.get``:

    detect (the caller's network) -> largest face -> 5 landmarks -> least-squares similarity onto the ArcFace template ->
    112 x 112 bilinear crop, (v - 127.5) / 127.5, RGB -> IResNet -> L2 normalisation.

The detector stays a callable of the caller's, by the convention of ``FaceCropper(detect_faces=...)`` (``ldm/modules/arcface_wrapper.py``), with
the five landmarks added: ``detect_faces(image_uint8_hwc_rgb) -> [(x, y, w, h, confidence, kps[5][2]), ...]``.  The similarity is a 2 x 3
host computation in fp64; warp, normalisation and channel padding are one kernel launch per image (``ops.face_align_crop``), and all crops
go through the recogniser (``adaface/iresnet.py``) in one batch."""
import numpy as np
import torch
import torch.nn.functional as F

from .. import ops

# insightface's ``arcface_dst``: left eye, right eye, nose tip, left and right mouth corner in the 112 x 112 crop
ARCFACE_TEMPLATE_112 = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655], [70.7299, 92.2041]],
                                dtype=np.float64)


def estimate_similarity(kps, template=ARCFACE_TEMPLATE_112):
    """Umeyama's least-squares similarity (rotation, uniform scale, shift; never a reflection) taking the landmarks ``kps`` [5, 2] onto
    ``template``.  fp64.  Returns (forward [2, 3]: image -> crop, inverse [2, 3]: crop -> image, what ``ops.face_align_crop`` reads)."""
    src, dst = np.asarray(kps, dtype=np.float64).reshape(-1, 2), np.asarray(template, dtype=np.float64).reshape(-1, 2)
    if src.shape != dst.shape:
        raise ValueError(f"estimate_similarity: {src.shape[0]} landmarks for a template of {dst.shape[0]}")
    mu_s, mu_d = src.mean(axis=0), dst.mean(axis=0)
    sc, dc = src - mu_s, dst - mu_d
    var_s = (sc ** 2).sum() / len(src)
    if not np.isfinite(var_s) or var_s <= 0:
        raise ValueError("estimate_similarity: the landmarks coincide (or are not finite)")
    U, S, Vt = np.linalg.svd(dc.T @ sc / len(src))
    d = np.ones(2)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:          # the best orthogonal fit would mirror: flip the weaker axis instead
        d[1] = -1.0
    R = U @ np.diag(d) @ Vt
    scale = float((S * d).sum() / var_s)
    if scale <= 0:
        raise ValueError("estimate_similarity: degenerate landmarks (no positive scale fits them)")
    fwd = np.concatenate([scale * R, (mu_d - scale * R @ mu_s)[:, None]], axis=1)
    Ri = R.T / scale
    inv = np.concatenate([Ri, (-Ri @ fwd[:, 2])[:, None]], axis=1)
    return np.ascontiguousarray(fwd), np.ascontiguousarray(inv)


def load_rgb_u8(image):
    """A path, a PIL image or a uint8 array ([H, W, 3] RGB, or [H, W] grey) -> a contiguous uint8 [H, W, 3] array; never resized."""
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8 or image.ndim not in (2, 3) or (image.ndim == 3 and image.shape[2] != 3):
            raise ValueError(f"an image array must be uint8 [H, W, 3] (RGB) or [H, W], got {image.dtype} {image.shape}")
        return np.ascontiguousarray(image if image.ndim == 3 else np.repeat(image[:, :, None], 3, axis=2))
    from PIL import Image
    if isinstance(image, (str, bytes)) or hasattr(image, "__fspath__"):
        with Image.open(image) as im:
            return np.array(im.convert("RGB"), dtype=np.uint8)
    if isinstance(image, Image.Image):
        return np.array(image.convert("RGB"), dtype=np.uint8)
    raise ValueError(f"an image must be a path, a PIL image or a uint8 array, got {type(image).__name__}")


class FaceIDExtractor:
    """``recogniser``: an ``IResNet`` on the GPU (``forward_nhwc`` is called), or any callable on the crops fp16 [N, 112, 112, 8] -> [N, 512].
    ``detect_faces``: the caller's detector (module docstring).  ``device``: where images are uploaded and cropped; by default the
    recogniser's."""
    crop_size = 112

    def __init__(self, recogniser, detect_faces, device=None):
        self.recogniser = recogniser
        self.detect_faces = detect_faces
        if device is None:
            p = next(iter(recogniser.parameters()), None) if hasattr(recogniser, "parameters") else None
            device = p.device if p is not None else "cuda"
        self.device = torch.device(device)

    @torch.no_grad()
    def extract(self, images, calc_avg=False, skip_non_faces=True):
        """-> (faceless_img_count, id_embs): unit-norm fp32 IDs [N_found, 512] in image order ([1, 512], their normalised mean, with
        ``calc_avg``), or None when no image shows a face.  An image without a face is counted and skipped, or raises ValueError with
        ``skip_non_faces=False``."""
        crops, faceless = [], 0
        for i, image in enumerate(images):
            rgb = load_rgb_u8(image)
            faces = self.detect_faces(rgb)
            if not faces:
                if not skip_non_faces:
                    raise ValueError(f"no face detected in {image if isinstance(image, str) else f'image #{i}'}")
                faceless += 1
                continue
            kps = max(faces, key=lambda f: f[2] * f[3])[5]                      # the largest face by box area
            inv = torch.from_numpy(estimate_similarity(kps)[1].astype(np.float32))[None]
            crops.append(ops.face_align_crop(torch.from_numpy(rgb).to(self.device), inv.to(self.device), self.crop_size))
        if not crops:
            return faceless, None
        run = getattr(self.recogniser, "forward_nhwc", self.recogniser)
        id_embs = F.normalize(run(torch.cat(crops, dim=0)).float(), p=2, dim=-1)
        if calc_avg:
            from .face_id_to_ada_prompt import Arc2Face_ID2AdaPrompt
            id_embs = Arc2Face_ID2AdaPrompt.average_id_embs(id_embs)
        return faceless, id_embs
