"""Repainting faces in a photo, host logic, CPU only (INTEGRATION.md "Repainting faces in a photo"): the crop rectangle, the face ellipses,
the fp64 restatement of the resampling rule against torch, the integer form of that rule the kernels use, the wrapper's refusals before
any GPU work and the C ABI's argument checks (which precede every launch, so they are observable without a GPU)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from adaface_dev_amd.adaface import face_repaint as R
from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper
from test_inpaint_host import _img, _mask, _vae, _wrapper


# ---------------------------------------------------------------------------------------------------------------- crop_region
def _inside(rect, H, W):
    x0, y0, cw, ch = rect
    return all(isinstance(v, int) for v in rect) and cw >= 1 and ch >= 1 and x0 >= 0 and y0 >= 0 and x0 + cw <= W and y0 + ch <= H


@pytest.mark.parametrize("work_hw", [(512, 512), (512, 768), (768, 512), (64, 128)])
def test_crop_region_reaches_the_aspect_ratio(work_hw):
    """In the interior of a large photo the rectangle has the working size's aspect ratio up to the rounding of its two sides (each by at
    most half a pixel), covers the padded region and is centred on it."""
    box = np.array([[1400.0, 900.0, 1700.0, 1320.0]])                # 300 x 420
    x0, y0, cw, ch = R.crop_region(box, (2000, 3000), work_hw, 0.25)
    Hs, Ws = work_hw
    assert abs(cw * Hs - ch * Ws) <= 0.5 * (Hs + Ws)
    pad = 0.25 * 420
    assert x0 <= 1400 - pad + 1 and y0 <= 900 - pad + 1 and x0 + cw >= 1700 + pad - 1 and y0 + ch >= 1320 + pad - 1
    assert abs((x0 + cw / 2) - 1550) <= 1 and abs((y0 + ch / 2) - 1110) <= 1
    assert min(cw - (300 + 2 * pad), ch - (420 + 2 * pad)) <= 1                       # only the shorter dimension grew


def test_crop_region_is_shifted_inside_at_each_border():
    H, W = 400, 600
    for box, edge in (([[5, 150, 65, 210]], "left"), ([[540, 150, 598, 210]], "right"), ([[250, 2, 310, 62]], "top"),
                      ([[250, 340, 310, 399]], "bottom")):
        x0, y0, cw, ch = R.crop_region(np.array(box, dtype=float), (H, W), (64, 64), 1.0)       # ~60 + 2 * 60 = 180 wide: sticks out
        assert _inside((x0, y0, cw, ch), H, W) and abs(cw - ch) <= 1 and 170 <= cw <= 182, edge
        assert {"left": x0 == 0, "right": x0 + cw == W, "top": y0 == 0, "bottom": y0 + ch == H}[edge], edge
        bx0, by0, bx1, by1 = box[0]
        assert x0 <= bx0 and y0 <= by0 and x0 + cw >= bx1 and y0 + ch >= by1, edge              # shifted, not clipped: the box stays inside


def test_crop_region_is_clipped_when_the_photo_is_smaller():
    assert R.crop_region(np.array([[10.0, 10.0, 90.0, 50.0]]), (60, 100), (64, 64), 0.5) == (0, 0, 100, 60)          # both dimensions
    x0, y0, cw, ch = R.crop_region(np.array([[100.0, 10.0, 140.0, 50.0]]), (60, 400), (64, 64), 0.5)                 # 80 x 80 wanted, H = 60
    assert (y0, ch) == (0, 60) and cw == 80 and x0 == 80                                                             # anisotropic
    assert R.crop_region(np.array([[3.2, 4.1, 3.3, 4.2]]), (9, 9), (64, 64), 0.0)[2:] == (1, 1)                      # never empty


def test_crop_region_is_inside_the_photo_over_a_sweep():
    rng = np.random.default_rng(5)
    for _ in range(2000):
        H, W = (int(v) for v in rng.integers(1, 700, 2))
        n = int(rng.integers(1, 4))
        c = rng.uniform(-0.2, 1.2, (n, 2)) * (W, H)
        half = rng.uniform(0.01, 0.6, (n, 2)) * (W, H)
        boxes = np.concatenate([c - half, c + half], axis=1)
        work = tuple(int(v) * 64 for v in rng.integers(1, 5, 2))
        pad = float(rng.uniform(0, 2))
        if boxes[:, 2].max() <= 0 or boxes[:, 3].max() <= 0 or boxes[:, 0].min() >= W or boxes[:, 1].min() >= H:
            with pytest.raises(ValueError, match="outside"):
                R.crop_region(boxes, (H, W), work, pad)
            continue
        assert _inside(R.crop_region(boxes, (H, W), work, pad), H, W), (boxes, H, W, work, pad)


def test_crop_region_refuses_bad_arguments():
    b = np.array([[1.0, 1.0, 5.0, 5.0]])
    for args in ((np.zeros((0, 4)), (9, 9), (64, 64), 0.5), (b, (9, 9), (64, 64), -0.1), (b, (0, 9), (64, 64), 0.5),
                 (np.array([[1.0, 1.0, np.nan, 5.0]]), (9, 9), (64, 64), 0.5)):
        with pytest.raises(ValueError):
            R.crop_region(*args)
    with pytest.raises(ValueError, match="all black"):
        R.mask_bbox(np.zeros((8, 8), dtype=bool))
    m = np.zeros((8, 9), dtype=bool)
    m[2, 3] = m[5, 7] = True
    assert R.mask_bbox(m).tolist() == [[3, 2, 8, 6]]


# ---------------------------------------------------------------------------------------------------------------- face_ellipses
FACES = [(100.0, 50.0, 40.0, 60.0, 0.99, None), (10.0, 20.0, 30.0, 20.0, 0.9, None)]


def test_face_ellipses_selection():
    e = R.face_ellipses(FACES)
    assert e.dtype == np.float32 and e.shape == (2, 4)
    assert np.allclose(e, [[120, 80, 1.3 * 20, 1.3 * 30], [25, 30, 1.3 * 15, 1.3 * 10]])
    assert np.allclose(R.face_ellipses(FACES, face_index=1, expand=2.0), [[25, 30, 30, 20]])
    assert np.allclose(R.face_ellipses(FACES, face_index=0, expand=1.0), [[120, 80, 20, 30]])
    assert np.allclose(R.ellipse_boxes(R.face_ellipses(FACES, 1, 2.0)), [[-5, 10, 55, 50]])


def test_face_ellipses_refusals():
    for none in ([], None, ()):
        with pytest.raises(R.NoFaceFound):
            R.face_ellipses(none)
    assert issubclass(R.NoFaceFound, ValueError) and issubclass(R.FaceDetectorMissing, ValueError)
    for bad in (2, -1, 1.0, True):
        with pytest.raises(ValueError, match="face_index") as ei:
            R.face_ellipses(FACES, face_index=bad)
        assert not isinstance(ei.value, R.NoFaceFound)
    with pytest.raises(ValueError, match="expand"):
        R.face_ellipses(FACES, expand=0.0)


# ---------------------------------------------------------------------------------------------------------------- the resampling rule
@pytest.mark.parametrize("n_in, n_out", [(37, 16), (13, 16), (16, 16), (100, 8), (900, 512), (512, 900), (64, 200)])
def test_resample_rule_matches_torch_antialias_fp64(n_in, n_out):
    """The fp64 restatement against F.interpolate(mode="bilinear", antialias=True) on CPU doubles: down, up and identity scales, on both
    axes at once (the other axis takes a second scale of the list)."""
    other_in, other_out = (23, 40) if n_in != n_out else (40, 40)
    x = torch.from_numpy(np.random.default_rng(n_in * 1000 + n_out).uniform(-1, 1, (2, 3, other_in, n_in)))
    ref = F.interpolate(x, size=(other_out, n_out), mode="bilinear", antialias=True, align_corners=False).numpy()
    got = R.resample2d(x.numpy(), (other_out, n_out))
    assert np.abs(got - ref).max() <= 2e-13
    if n_in == n_out:
        assert np.array_equal(R.resample_matrix(n_in, n_out), np.eye(n_in))
        assert np.array_equal(got, x.numpy())


def _integer_form(n_in, n_out):
    """The kernels' form of the rule (include/adaface_hip.h): everything over 2 n_out, D = 2 max(n_in, n_out), integer tap ranges and
    integer un-normalised weights m_k = max(0, D - |2 n_out k + n_out - n_in (2 i + 1)|); the weight is m_k / sum(m)."""
    m = np.zeros((n_out, n_in), dtype=np.float64)
    step, D = 2 * n_out, 2 * max(n_in, n_out)
    for i in range(n_out):
        cnum = n_in * (2 * i + 1)
        lo = max(0, (cnum - D + n_out)) // step
        hi = min(n_in, (cnum + D + n_out) // step)
        ms = [max(0, D - abs(step * k + n_out - cnum)) for k in range(lo, hi)]
        assert sum(ms) > 0
        m[i, lo:hi] = np.array(ms, dtype=np.float64) / sum(ms)
    return m


@pytest.mark.parametrize("n_in, n_out", [(37, 16), (13, 16), (16, 16), (100, 8), (8, 100), (900, 512), (512, 900), (3, 7), (1, 5), (5, 1)])
def test_integer_form_of_the_rule_is_the_rule(n_in, n_out):
    """The integer form is exact up to its one division; the fp64 rule rounds s and c = s (i + 0.5) <= n_in (2^-53 n_in each), the
    difference k - c + 0.5, the division by sup and the normalisation: 8 n_in 2^-52 bounds the sum generously."""
    assert np.abs(_integer_form(n_in, n_out) - R.resample_matrix(n_in, n_out)).max() <= 8 * n_in * 2.0 ** -52
    if n_in == n_out:
        assert np.array_equal(_integer_form(n_in, n_out), np.eye(n_in))


def test_resample_taps_is_a_run_time_quantity():
    assert R.resample_taps(16, 16) == 1 and R.resample_taps(13, 16) == 2 and 24 <= R.resample_taps(100, 8) <= 26


def test_alpha_and_paste_back_restatements():
    a, r = R.alpha_mask_f64(np.array([[4.3, 4.5, 3.0, 2.0]]), (9, 9), 0.25)
    assert a[4, 4] == 1 and a[0, 0] == 0 and r.shape == (1, 9, 9) and 0 < a[4, 1] < 1
    assert np.array_equal(R.alpha_mask_f64(np.zeros((0, 4)), (3, 5), 0.25)[0], np.zeros((3, 5)))
    hard = R.alpha_mask_f64(np.array([[4.3, 4.5, 3.0, 2.0]]), (9, 9), 0.0)[0]
    assert set(np.unique(hard)) == {0.0, 1.0} and hard[4, 1] == 1 and hard[4, 0] == 0
    photo = np.random.default_rng(1).integers(0, 256, (9, 9, 3), dtype=np.uint8)
    dec = np.random.default_rng(2).uniform(-1.5, 1.5, (2, 3, 4, 4))
    out = R.paste_back_f64(dec, photo, a, (2, 3, 4, 4))
    keep = np.ones((9, 9), dtype=bool)
    keep[3:7, 2:6] = a[3:7, 2:6] == 0
    assert np.array_equal(out[:, keep], np.repeat(photo[None].astype(np.float64), 2, 0)[:, keep])
    ones = R.paste_back_f64(dec, photo, np.ones((9, 9)), (2, 3, 4, 4))[:, 3:7, 2:6]
    assert np.allclose(ones, 255 * np.clip(dec / 2 + 0.5, 0, 1).transpose(0, 2, 3, 1), atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------- wrapper refusals
def _detector(rgb):
    raise AssertionError("the detector must not run before the refusals")


def test_face_mask_without_a_detector_is_refused():
    """forward(photo, ..., mask_image="face") without a detector: FaceDetectorMissing, before anything else."""
    pe = torch.zeros(1, 77, 64)
    w = _wrapper("inpaint", vae=_vae())
    assert w.face_detector is None
    for kw in (dict(), dict(crop_padding=0.5)):
        with pytest.raises(R.FaceDetectorMissing, match="face_detector"):
            w(_img(), None, prompt_embeds=(pe, pe), out_image_count=1, mask_image="face", **kw)


def test_wrapper_takes_the_detector_from_the_extractor():
    import types
    from adaface_dev_amd.adaface.arc2face_models import clip_text_config
    from adaface_dev_amd import TINY_UNET_CONFIG
    cc = clip_text_config(hidden_size=64, num_attention_heads=1, num_hidden_layers=1, intermediate_size=128)
    kw = dict(pipeline_name="inpaint", clip_config=cc, unet_config=dict(TINY_UNET_CONFIG), device="cpu", vae=_vae())
    ext = types.SimpleNamespace(detect_faces=_detector)
    assert AdaFaceWrapper(face_id_extractor=ext, **kw).face_detector is _detector
    other = lambda rgb: []
    assert AdaFaceWrapper(face_id_extractor=ext, face_detector=other, **kw).face_detector is other


def test_wrapper_repaint_refuses_before_any_gpu_work():
    pe = torch.zeros(1, 77, 64)
    w = _wrapper("inpaint", vae=_vae())
    w.face_detector = _detector
    call = lambda *a, **kw: w(*a, None, prompt_embeds=(pe, pe), out_image_count=1, **kw)
    with pytest.raises(ValueError, match="'face'"):
        call(_img(), mask_image="faces")
    for kw, match in ((dict(crop_padding=-0.1), "crop_padding"), (dict(crop_padding=float("nan")), "crop_padding"),
                      (dict(crop_padding="0.5"), "crop_padding"), (dict(face_mask_expand=-1.0), "face_mask_expand"),
                      (dict(face_mask_expand=0.0), "face_mask_expand"), (dict(face_mask_feather=-0.25), "face_mask_feather"),
                      (dict(face_index=-1), "face_index"), (dict(face_index=0.5), "face_index"),
                      (dict(crop_padding=0.5, work_size=(100, 64)), "work_size"), (dict(crop_padding=0.5, work_size=(64, 2048)), "work_size"),
                      (dict(crop_padding=0.5, work_size=(0, 64)), "work_size"), (dict(crop_padding=0.5, work_size=64), "work_size"),
                      (dict(crop_padding=0.5, work_size=(64, 64, 64)), "work_size"), (dict(work_size=(64, 64)), "work_size"),
                      (dict(crop_padding=0.5, ref_img_strength=1.5), "strength")):
        with pytest.raises(ValueError, match=match):
            call(_img(), mask_image="face", **kw)
    with pytest.raises(ValueError, match="one photo"):
        call([_img(), _img()], mask_image="face", crop_padding=0.5)
    with pytest.raises(ValueError, match="one photo"):
        call([_img(), _img()], mask_image=_mask(64, 64, 255), crop_padding=0.5)
    with pytest.raises(ValueError, match="one mask"):
        call(_img(), mask_image=[_mask(64, 64, 255)] * 2, crop_padding=0.5)
    with pytest.raises(ValueError, match="face_index"):
        call(_img(), mask_image=_mask(64, 64, 255), face_index=0)
    with pytest.raises(ValueError, match="all black"):
        call(_img(), mask_image=_mask(64, 64, 0), crop_padding=0.5)
    with pytest.raises(ValueError, match="PIL"):
        call(_img(), mask_image=np.zeros((64, 64), dtype=np.uint8), crop_padding=0.5)
    w.face_detector = lambda rgb: []
    with pytest.raises(R.NoFaceFound):
        call(np.zeros((50, 70, 3), dtype=np.uint8), mask_image="face", crop_padding=0.5)
    w.face_detector = lambda rgb: [(10.0, 10.0, 20.0, 20.0, 0.9, None)]
    with pytest.raises(ValueError, match="face_index") as ei:
        call(_img(), mask_image="face", crop_padding=0.5, face_index=1)
    assert not isinstance(ei.value, R.NoFaceFound)
    with pytest.raises(ValueError, match="1024"):                                   # whole-photo mode keeps the VAE's size limit
        call(np.zeros((64, 1100, 3), dtype=np.uint8), mask_image="face")


def test_other_pipelines_refuse_the_repaint_keywords():
    pe = torch.zeros(1, 77, 64)
    for name in ("text2img", "img2img"):
        w = _wrapper(name)
        w.vae = _vae()
        first = _img() if name == "img2img" else torch.zeros(1, 4, 8, 8)
        for kw, match in ((dict(crop_padding=0.5), "crop_padding"), (dict(face_index=0), "face_index"), (dict(work_size=(64, 64)), "work_size"),
                          (dict(mask_image="face"), "mask_image")):
            with pytest.raises(ValueError, match=match):
                w(first, None, prompt_embeds=(pe, pe), out_image_count=1, **kw)


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_refuses_bad_repaint_arguments_before_any_launch():
    """Argument validation precedes the launch, so it is observable without a GPU (the device pointers are never dereferenced)."""
    from adaface_dev_amd import _lib
    L = _lib.lib()
    E = _lib.AF_E_BADARG
    named = lambda name: name.encode() in L.af_last_error()
    p = 4096
    #            ellipses alpha F  H   W   feather
    for args in ((p, None, 1, 64, 64, 0.25), (None, p, 1, 64, 64, 0.25), (p, p, -1, 64, 64, 0.25), (p, p, 1, 0, 64, 0.25), (p, p, 1, 64, 0, 0.25),
                 (p, p, 1, 64, 64, -0.5), (p, p, 1, 64, 64, float("nan")), (p, p, 1, 32768, 32768, 0.25), (p, p, 1, 26755, 26755, 0.25)):
        assert L.af_face_alpha_mask(*args, None) == E and named("af_face_alpha_mask"), args
    #        photo alpha image mask  H    W    x0 y0 cw  ch  Hs  Ws  thr
    good = [p, p, p, p, 100, 120, 10, 20, 50, 40, 64, 32, 0.5]
    for idx, val in ((0, None), (1, None), (2, None), (3, None), (4, 0), (5, -3), (10, 60), (11, 36), (10, 0), (11, -8),
                     (6, -1), (7, -1), (8, 0), (9, 0), (8, 111), (9, 81), (6, 120), (7, 2 ** 31 - 1), (2, p + 2)):
        args = list(good)
        args[idx] = val
        assert L.af_crop_resize_u8(*args, None) == E and named("af_crop_resize_u8"), args
    assert L.af_crop_resize_u8(p, p, p, p, 26755, 26755, 0, 0, 8, 8, 8, 8, 0.5, None) == E and named("af_crop_resize_u8")       # H W 3 >= 2^31
    assert L.af_crop_resize_u8(p, p, p, p, 64, 64, 0, 0, 8, 8, 32768, 32768, 0.5, None) == E and named("af_crop_resize_u8")
    #        decoded photo alpha out B  Hs  Ws  H    W    x0 y0 cw  ch
    good = [p, p, p, p, 2, 64, 32, 100, 120, 10, 20, 50, 40]
    for idx, val in ((0, None), (1, None), (2, None), (3, None), (4, 0), (5, 0), (6, -1), (7, 0), (8, 0), (9, -1), (10, -1), (11, 0), (12, 0),
                     (11, 111), (12, 81), (9, 2 ** 31 - 1), (10, 100)):
        args = list(good)
        args[idx] = val
        assert L.af_paste_back_u8(*args, None) == E and named("af_paste_back_u8"), args
    for B, H, W, Hs, Ws in ((1, 26755, 26755, 8, 8), (4, 14000, 14000, 8, 8), (3, 64, 64, 16384, 16384)):       # H W 3, B H W 3, B 3 Hs Ws >= 2^31
        assert L.af_paste_back_u8(p, p, p, p, B, Hs, Ws, H, W, 0, 0, 8, 8, None) == E and named("af_paste_back_u8"), (B, H, W, Hs, Ws)


def test_ops_wrappers_check_their_tensors():
    """dtype, device, contiguity and shape checks of the ops wrappers (CPU tensors are refused before the library is called)."""
    from adaface_dev_amd import ops
    photo, alpha = torch.zeros(8, 8, 3, dtype=torch.uint8), torch.zeros(8, 8)
    with pytest.raises(RuntimeError, match="face_alpha_mask.ellipses"):
        ops.face_alpha_mask(torch.zeros(1, 4), (8, 8), 0.25)
    with pytest.raises(RuntimeError, match="crop_resize_u8.photo"):
        ops.crop_resize_u8(photo, alpha, (0, 0, 8, 8), (8, 8))
    with pytest.raises(RuntimeError, match="paste_back_u8.photo"):
        ops.paste_back_u8(torch.zeros(1, 3, 8, 8), photo, alpha, (0, 0, 8, 8))
