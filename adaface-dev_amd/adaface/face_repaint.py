"""Host side of "repaint the faces of a photo" (INTEGRATION.md "Repainting faces in a photo"): which ellipses make the face mask, which
rectangle of the photo goes through the VAE and the U-Net, and an fp64 restatement of the resampling rule the kernels of
``csrc/af_repaint.hip`` implement.  Pure numpy / Python: nothing here touches the GPU.

The pipeline itself is ``AdaFaceWrapper.forward(photo, ..., mask_image="face", crop_padding=...)`` under ``pipeline_name="inpaint"``:
ellipses -> ``ops.face_alpha_mask`` -> ``crop_region`` -> ``ops.crop_resize_u8`` -> ``inpaint_latents`` + ``sample_inpaint`` ->
``vae.decode`` -> ``ops.paste_back_u8``."""
import numpy as np


class NoFaceFound(ValueError):
    """The detector returned no face for the photo (``mask_image="face"``)."""


class FaceDetectorMissing(ValueError):
    """``mask_image="face"`` on a wrapper built without ``face_detector`` (and without a ``face_id_extractor`` to take one from)."""


def face_ellipses(faces, face_index=None, expand=1.3):
    """``faces``: ``FaceIDExtractor``'s detector contract, [(x, y, w, h, confidence, kps), ...], best first.  -> fp32 [F, 4] rows
    (cx, cy, rx, ry) = (x + w/2, y + h/2, expand w/2, expand h/2) in photo pixels: all faces (``face_index=None``) or the k-th.
    ``expand`` defaults to 1.3 because RetinaFace boxes are tight around the face.  No faces: ``NoFaceFound``; an index outside
    [0, len(faces)): ``ValueError``."""
    faces = list(faces) if faces is not None else []
    if not faces:
        raise NoFaceFound("no face detected in the photo")
    if not expand > 0:
        raise ValueError(f"expand must be positive, got {expand!r}")
    if face_index is not None:
        if isinstance(face_index, bool) or not isinstance(face_index, (int, np.integer)) or not 0 <= face_index < len(faces):
            raise ValueError(f"face_index must be an integer in [0, {len(faces)}) for the {len(faces)} detected face(s), got {face_index!r}")
        faces = [faces[int(face_index)]]
    rows = []
    for f in faces:
        x, y, w, h = (float(v) for v in f[:4])
        if not (w > 0 and h > 0):
            raise ValueError(f"a detected face has an empty box: {(x, y, w, h)}")
        rows.append((x + w / 2, y + h / 2, expand * w / 2, expand * h / 2))
    return np.asarray(rows, dtype=np.float32).reshape(-1, 4)


def ellipse_boxes(ellipses):
    """[F, 4] (cx, cy, rx, ry) -> [F, 4] corner boxes (x0, y0, x1, y1), fp64."""
    e = np.asarray(ellipses, dtype=np.float64).reshape(-1, 4)
    return np.stack([e[:, 0] - e[:, 2], e[:, 1] - e[:, 3], e[:, 0] + e[:, 2], e[:, 1] + e[:, 3]], axis=1)


def mask_bbox(mask):
    """A boolean [H, W] mask -> its bounding box [[x0, y0, x1, y1]] (x1, y1 exclusive); nothing set: ``ValueError``."""
    mask = np.asarray(mask, dtype=bool)
    ys, xs = np.flatnonzero(mask.any(axis=1)), np.flatnonzero(mask.any(axis=0))
    if ys.size == 0:
        raise ValueError("the mask is all black: there is nothing to repaint")
    return np.array([[xs[0], ys[0], xs[-1] + 1, ys[-1] + 1]], dtype=np.float64)


def crop_region(boxes, photo_hw, work_hw, padding):
    """The rectangle of the photo that is resampled to the working size (restated from diffusers' ``padding_mask_crop``, not pinned; the
    padding here is relative to the region, diffusers' is in pixels).  ``boxes``: [N, 4] corner boxes (x0, y0, x1, y1) -- the expanded
    face boxes (``ellipse_boxes``) or a mask's bounding box (``mask_bbox``); ``photo_hw`` = (H, W); ``work_hw`` = (Hs, Ws).
      1. the union of the boxes, clipped to the photo;
      2. padded on every side by ``padding`` x its longer side;
      3. the shorter dimension grown symmetrically until cw / ch = Ws / Hs;
      4. rounded to integers;
      5. shifted inside the photo where it sticks out;
      6. a dimension still larger than the photo is clipped to it (the resize is then anisotropic, as in diffusers).
    -> (x0, y0, cw, ch), integers with cw, ch >= 1, inside the photo."""
    H, W = (int(v) for v in photo_hw)
    Hs, Ws = (int(v) for v in work_hw)
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    if H < 1 or W < 1 or Hs < 1 or Ws < 1:
        raise ValueError(f"photo_hw and work_hw must be positive, got {photo_hw!r}, {work_hw!r}")
    if b.shape[0] == 0 or not np.isfinite(b).all():
        raise ValueError("crop_region needs at least one finite box")
    if not padding >= 0:
        raise ValueError(f"padding must be >= 0, got {padding!r}")
    x0, y0 = max(0.0, b[:, 0].min()), max(0.0, b[:, 1].min())
    x1, y1 = min(float(W), b[:, 2].max()), min(float(H), b[:, 3].max())
    if x1 <= x0 or y1 <= y0:
        raise ValueError(f"the region {tuple(b.min(0)[:2]) + tuple(b.max(0)[2:])} lies outside the {W} x {H} photo")
    pad = padding * max(x1 - x0, y1 - y0)
    cx, cy, cw, ch = (x0 + x1) / 2, (y0 + y1) / 2, x1 - x0 + 2 * pad, y1 - y0 + 2 * pad
    if cw * Hs < ch * Ws:
        cw = ch * Ws / Hs
    else:
        ch = cw * Hs / Ws
    out = []
    for c, n, lim in ((cx, cw, W), (cy, ch, H)):
        n_i = max(1, int(round(n)))
        lo = int(round(c - n / 2))
        if n_i >= lim:
            lo, n_i = 0, lim
        else:
            lo = min(max(lo, 0), lim - n_i)
        out.append((lo, n_i))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def check_work_size(work_size, max_side):
    """``work_size`` = (W, H) in pixels, both multiples of 64 from 64 to ``max_side`` -> (Hs, Ws); else ``ValueError``."""
    try:
        W, H = (int(s) for s in work_size)
        exact = all(float(s) == int(s) for s in work_size)
    except (TypeError, ValueError):
        raise ValueError(f"work_size must be (W, H) in pixels, got {work_size!r}") from None
    if not exact or W % 64 or H % 64 or not (64 <= W <= max_side and 64 <= H <= max_side):
        raise ValueError(f"work_size sides must be multiples of 64 from 64 to {max_side} pixels, got {work_size!r}")
    return H, W


# ------------------------------------------------------------------------------------------------ fp64 restatements (tests, documentation)
def resample_matrix(n_in, n_out):
    """fp64 [n_out, n_in]: one axis of torch's ``F.interpolate(mode="bilinear", antialias=True, align_corners=False)``.
    s = n_in / n_out, sup = max(s, 1), c = s (i + 0.5); taps k in [max(0, int(c - sup + 0.5)), min(n_in, int(c + sup + 0.5)));
    weight max(0, 1 - |(k - c + 0.5) / sup|), normalised by the sum over the taps.  The identity at n_in == n_out."""
    s = n_in / n_out
    sup = max(s, 1.0)
    m = np.zeros((n_out, n_in), dtype=np.float64)
    for i in range(n_out):
        c = s * (i + 0.5)
        lo, hi = max(0, int(c - sup + 0.5)), min(n_in, int(c + sup + 0.5))
        k = np.arange(lo, hi, dtype=np.float64)
        w = np.maximum(0.0, 1.0 - np.abs((k - c + 0.5) / sup))
        m[i, lo:hi] = w / w.sum()
    return m


def resample_taps(n_in, n_out):
    """The largest number of taps with a non-zero weight over the outputs of one axis (for error bounds)."""
    return int((resample_matrix(n_in, n_out) > 0).sum(axis=1).max())


def resample2d(x, out_hw):
    """fp64 [..., h, w] -> [..., Ho, Wo] by ``resample_matrix`` along x, then y."""
    x = np.asarray(x, dtype=np.float64)
    my, mx = resample_matrix(x.shape[-2], out_hw[0]), resample_matrix(x.shape[-1], out_hw[1])
    return my @ (x @ mx.T)


def alpha_mask_f64(ellipses, photo_hw, feather):
    """fp64 restatement of ``ops.face_alpha_mask`` -> (alpha [H, W], r [F, H, W])."""
    H, W = photo_hw
    e = np.asarray(ellipses, dtype=np.float64).reshape(-1, 4)
    ys, xs = np.arange(H, dtype=np.float64)[:, None] + 0.5, np.arange(W, dtype=np.float64)[None, :] + 0.5
    r = np.stack([np.sqrt(((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2) for cx, cy, rx, ry in e]) if len(e) else np.zeros((0, H, W))
    if feather > 0:
        t = np.clip((1.0 - r) / feather, 0.0, 1.0)
        a = t * t * (3.0 - 2.0 * t)
    else:
        a = (r <= 1.0).astype(np.float64)
    return (a.max(axis=0) if len(e) else np.zeros((H, W))), r


def paste_back_f64(decoded, photo_u8, alpha, rect):
    """fp64 restatement of ``ops.paste_back_u8`` BEFORE rounding: decoded [B, 3, Hs, Ws], photo [H, W, 3], alpha [H, W] -> [B, H, W, 3]."""
    x0, y0, cw, ch = rect
    dec = np.asarray(decoded, dtype=np.float64)
    p = np.asarray(photo_u8, dtype=np.float64)
    out = np.repeat(p[None], dec.shape[0], axis=0)
    g = 255.0 * np.clip(resample2d(dec, (ch, cw)) / 2 + 0.5, 0.0, 1.0)                       # [B, 3, ch, cw]
    a = np.asarray(alpha, dtype=np.float64)[y0:y0 + ch, x0:x0 + cw, None]
    out[:, y0:y0 + ch, x0:x0 + cw] = a * g.transpose(0, 2, 3, 1) + (1.0 - a) * p[y0:y0 + ch, x0:x0 + cw]
    return out
