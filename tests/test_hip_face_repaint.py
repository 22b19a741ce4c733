"""Repainting faces in a photo on the GPU (INTEGRATION.md "Repainting faces in a photo"): the three kernels of csrc/af_repaint.hip against
fp64 restatements computed on the CPU (adaface/face_repaint.py, themselves pinned to torch in test_face_repaint_host.py), and the wrapper's
photo-level inpaint path end to end on the reduced-width U-Net and VAE of the inpaint tests, with a stub detector.

u = 2^-24 is fp32's unit roundoff throughout."""
import numpy as np
import pytest
import torch
from PIL import Image

from adaface_dev_amd.adaface import face_repaint as R
from test_hip_img2img import _pil, _unet_cfg
from test_vae_oracle import VAE_SMALL

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- face_alpha_mask
ELLIPSES = {  # (H, W) -> three ellipses: two overlapping, the third partly outside the photo
    (53, 71): [(30.3, 20.7, 14.2, 9.6), (40.1, 26.2, 10.5, 12.3), (66.4, 48.9, 9.7, 8.2)],
    (64, 64): [(20.3, 20.7, 14.2, 9.6), (30.1, 26.2, 10.5, 12.3), (60.4, 58.9, 9.7, 8.2)],
}


@pytest.mark.parametrize("hw", list(ELLIPSES))
@pytest.mark.parametrize("nf", [0, 1, 3])
@pytest.mark.parametrize("feather", [0.0, 0.25])
def test_face_alpha_mask(dev, hw, nf, feather):
    """Error of r in fp32: x + 0.5 is exact; d = x + 0.5 - cx, d / rx and its square round once each (the square carries 2 (u + u) + u =
    5 u), the sum of the two squares 6 u, the correctly rounded square root halves that and adds its own: |r32 - r64| <= 4 u r.  Then
    1 - r rounds by at most u phi where t is not clamped, the division by phi makes that u and adds u t, and t t (3 - 2 t) adds at most
    4 u: 6 u in all, which is (1.5 / phi) 4 u phi <= (1.5 / phi) 4 u for phi <= 1.  With d alpha / d r <= 1.5 / phi (the smoothstep's
    slope is at most 1.5, d t / d r = 1 / phi):  |alpha - alpha64| <= (1.5 / phi) dr,  dr = 8 u max(r, 1).
    Farther than dr outside r = 1 the clamp gives t = 0 and alpha = 0 exactly; farther than dr inside r = 1 - phi it gives t = 1 and
    alpha = 1 exactly.  phi = 0: alpha = (r <= 1), compared wherever |r64 - 1| > dr -- and the inputs leave no pixel within dr of 1."""
    from adaface_dev_amd import ops
    H, W = hw
    e = np.asarray(ELLIPSES[hw][:nf], dtype=np.float32).reshape(-1, 4)
    got = ops.face_alpha_mask(torch.from_numpy(e).to(dev), (H, W), feather).cpu().numpy().astype(np.float64)
    ref, r = R.alpha_mask_f64(e, (H, W), feather)                     # from the fp32 ellipses, as the kernel reads them
    assert got.shape == (H, W)
    if nf == 0:
        assert np.array_equal(got, np.zeros((H, W)))
        return
    dr = 8 * U * np.maximum(r, 1.0)
    if feather == 0:
        assert not (np.abs(r - 1.0) <= dr).any()                      # no pixel is left out of the comparison
        assert np.array_equal(got, ref)
        assert 0 < ref.mean() < 1
        return
    err = np.abs(got - ref)
    print(f"face_alpha_mask {hw} F={nf}: max |alpha - alpha64| = {err.max():.3e}, bound {1.5 / feather * 8 * U:.3e}")
    assert (err <= (1.5 / feather) * dr.max(axis=0)).all()
    outside, inside = (r > 1.0 + dr).all(axis=0), (r < 1.0 - feather - dr).any(axis=0)
    assert outside.any() and inside.any() and (~outside & ~inside).any()
    assert np.array_equal(got[outside], np.zeros(outside.sum())) and np.array_equal(got[inside], np.ones(inside.sum()))


# ---------------------------------------------------------------------------------------------------------------- crop_resize_u8 / paste_back_u8
# (H, W, rect = (x0, y0, cw, ch), (Hs, Ws)): widths with W % 4 in {0, 1, 3}; interior, the four corners, the whole photo; per-axis scales
# 37 -> 16, 13 -> 16, 16 -> 16, 100 -> 8 and anisotropic pairs; more than one workgroup (Ws = 40 > 32 columns, Hs = 48 > 32 rows).
CASES = {
    "interior_37to16": (110, 120, (11, 7, 37, 37), (16, 16)),
    "topleft_13to16": (103, 121, (0, 0, 13, 13), (16, 16)),
    "topright_16to16": (101, 123, (123 - 16, 0, 16, 16), (16, 16)),
    "bottomleft_100to8": (110, 120, (0, 10, 100, 100), (8, 8)),
    "bottomright_aniso": (103, 121, (121 - 37, 103 - 13, 37, 13), (16, 16)),
    "whole_16to16_two_blocks": (48, 40, (0, 0, 40, 48), (48, 40)),
    "whole_aniso": (37, 100, (0, 0, 100, 37), (16, 8)),
    "interior_odd_width_16to16": (61, 123, (50, 30, 16, 16), (16, 16)),
}
THR = 1.0 / 255.0


def _photo(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _case_alpha(H, W, rect):
    """A soft ellipse in the top left quarter of the rectangle (zeros, ones and a feather band; latent cells of both kinds), as fp32."""
    x0, y0, cw, ch = rect
    return R.alpha_mask_f64(np.array([[x0 + 0.3 * cw, y0 + 0.32 * ch, 0.18 * cw, 0.17 * ch]]), (H, W), 0.4)[0].astype(np.float32)


def _delta(n_in_hw, n_out_hw):
    """delta = 255 (n_y + n_x + 8) 2^-23 for n taps per axis.  Each normalised weight is ONE correctly rounded fp32 division of two exact
    integers (relative error u / 2), so the weights of an axis contribute at most 255 u / 2 per axis; a sum of n products carries n + 1
    roundings of at most 255 u each along x and again along y: 255 u (n_x + n_y + 3).  The clamp is exact.  For the paste-back the
    same sums are over |d| <= 1.5 scaled by 127.5, and d / 2 + 0.5, the product by 255, alpha g, 1 - alpha, (1 - alpha) p and their sum add
    at most 6 roundings of 255 u.  Both stay below 255 (n_y + n_x + 8) 2 u."""
    ny, nx = R.resample_taps(n_in_hw[0], n_out_hw[0]), R.resample_taps(n_in_hw[1], n_out_hw[1])
    return 255.0 * (ny + nx + 8) * 2.0 ** -23


def _crop_ref(photo, alpha, rect, work_hw):
    x0, y0, cw, ch = rect
    v = R.resample2d(photo[y0:y0 + ch, x0:x0 + cw].transpose(2, 0, 1), work_hw).transpose(1, 2, 0)
    a = R.resample2d(alpha[y0:y0 + ch, x0:x0 + cw], work_hw)
    Hs, Ws = work_hw
    blockmax = a.reshape(Hs // 8, 8, Ws // 8, 8).max(axis=(1, 3))
    return np.clip(v, 0, 255), blockmax


def _run_crop(dev, photo, alpha, rect, work_hw):
    from adaface_dev_amd import ops
    image, mask_lat = ops.crop_resize_u8(torch.from_numpy(photo).to(dev), torch.from_numpy(alpha).to(dev), rect, work_hw, THR)
    Hs, Ws = work_hw
    assert image.shape == (1, Hs, Ws, 3) and image.dtype == torch.uint8 and mask_lat.shape == (1, 1, Hs // 8, Ws // 8)
    return image[0].cpu().numpy(), mask_lat[0, 0].cpu().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_crop_resize_u8(dev, name):
    """|image - v64| <= 0.5 + delta (``_delta``) against the fp64 value before rounding; at scale 1 the slice bit for bit; mask_lat equal
    to the fp64 rule, with no block maximum of the reference within 1e-5 of thr (asserted, so no cell is left out)."""
    H, W, rect, work_hw = CASES[name]
    x0, y0, cw, ch = rect
    photo, alpha = _photo(H, W, seed=len(name)), _case_alpha(H, W, rect)
    image, mask_lat = _run_crop(dev, photo, alpha, rect, work_hw)
    v, blockmax = _crop_ref(photo, alpha.astype(np.float64), rect, work_hw)
    err = np.abs(image.astype(np.float64) - v).max()
    print(f"crop_resize_u8 {name}: max |image - v64| = {err:.6f}, bound 0.5 + {_delta((ch, cw), work_hw):.2e}")
    assert err <= 0.5 + _delta((ch, cw), work_hw)
    if (ch, cw) == tuple(work_hw):
        assert np.array_equal(image, photo[y0:y0 + ch, x0:x0 + cw])
    assert not (np.abs(blockmax - THR) <= 1e-5).any()
    assert np.array_equal(mask_lat, (blockmax >= THR).astype(np.float32))


@pytest.mark.parametrize("name", ["interior_37to16", "whole_16to16_two_blocks", "whole_aniso"])
def test_crop_resize_u8_mask_edge_cases(dev, name):
    """alpha all 0 -> no cell; all 1 -> every cell; a single non-zero pixel at a block corner -> the cells the fp64 rule gives (at scale 1:
    that block alone)."""
    H, W, rect, work_hw = CASES[name]
    x0, y0, cw, ch = rect
    photo = _photo(H, W, seed=3)
    Hs, Ws = work_hw
    assert not _run_crop(dev, photo, np.zeros((H, W), dtype=np.float32), rect, work_hw)[1].any()
    assert _run_crop(dev, photo, np.ones((H, W), dtype=np.float32), rect, work_hw)[1].all()
    one = np.zeros((H, W), dtype=np.float32)
    py, px = y0 + (8 * ch) // Hs - (1 if Hs > 8 else ch // 2), x0 + (8 * cw) // Ws - (1 if Ws > 8 else cw // 2)
    one[py, px] = 1.0          # the source pixel under the last row / column of output block (0, 0) (the middle, for a one-block output)
    mask_lat = _run_crop(dev, photo, one, rect, work_hw)[1]
    blockmax = _crop_ref(photo, one.astype(np.float64), rect, work_hw)[1]
    assert not (np.abs(blockmax - THR) <= 1e-5).any()
    assert np.array_equal(mask_lat, (blockmax >= THR).astype(np.float32)) and mask_lat[0, 0] == 1
    if (ch, cw) == tuple(work_hw):
        assert mask_lat.sum() == 1


def _decoded(B, work_hw, seed):
    return np.random.default_rng(seed).uniform(-1.5, 1.5, (B, 3) + tuple(work_hw)).astype(np.float32)      # values outside [-1, 1] too


@pytest.mark.parametrize("name,B", [(n, 3 if i % 2 else 1) for i, n in enumerate(CASES)])
def test_paste_back_u8(dev, name, B):
    """decoded (Hs, Ws) -> the rectangle (so 100 -> 8 of the crop is 8 -> 100 here): outside the rectangle and wherever alpha == 0 the photo's
    bytes; elsewhere |out - v64| <= 0.5 + delta (``_delta``)."""
    from adaface_dev_amd import ops
    H, W, rect, work_hw = CASES[name]
    x0, y0, cw, ch = rect
    photo, alpha, dec = _photo(H, W, seed=len(name) + 50), _case_alpha(H, W, rect), _decoded(B, work_hw, seed=len(name))
    out = ops.paste_back_u8(torch.from_numpy(dec).to(dev), torch.from_numpy(photo).to(dev), torch.from_numpy(alpha).to(dev), rect)
    assert out.shape == (B, H, W, 3) and out.dtype == torch.uint8
    out = out.cpu()
    keep = np.ones((H, W), dtype=bool)
    keep[y0:y0 + ch, x0:x0 + cw] = alpha[y0:y0 + ch, x0:x0 + cw] == 0
    assert keep.any() or rect == (0, 0, W, H)
    keep_t, photo_t = torch.from_numpy(keep), torch.from_numpy(photo)
    for b in range(B):
        assert torch.equal(out[b][keep_t], photo_t[keep_t])
    v = R.paste_back_f64(dec, photo, alpha.astype(np.float64), rect)
    err = np.abs(out.numpy().astype(np.float64) - v).max()
    print(f"paste_back_u8 {name} B={B}: max |out - v64| = {err:.6f}, bound 0.5 + {_delta(work_hw, (ch, cw)):.2e}")
    assert err <= 0.5 + _delta(work_hw, (ch, cw))
    assert (out.numpy()[:, ~keep] != photo[~keep]).any()


@pytest.mark.parametrize("H,W,B", [(48, 40, 3), (24, 37, 1)])
def test_paste_back_u8_alpha_one_is_to_pil(dev, H, W, B):
    """alpha = 1 everywhere, the whole photo, scale 1: what ``_to_pil`` computes, ((d / 2 + 0.5).clamp(0, 1) * 255).round() in fp32 on the
    CPU, bit for bit (wide and scalar forms)."""
    from adaface_dev_amd import ops
    dec = torch.from_numpy(_decoded(B, (H, W), seed=H))
    photo = torch.from_numpy(_photo(H, W, seed=W))
    out = ops.paste_back_u8(dec.to(dev), photo.to(dev), torch.ones(H, W, device=dev), (0, 0, W, H)).cpu()
    ref = ((dec / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1)
    assert torch.equal(out, ref)
    out = ops.paste_back_u8(dec.to(dev), photo.to(dev), torch.zeros(H, W, device=dev), (0, 0, W, H)).cpu()
    assert torch.equal(out, photo[None].expand(B, H, W, 3))


# ---------------------------------------------------------------------------------------------------------------- wrapper, end to end
FACES = [(70.0, 40.0, 16.0, 20.0, 0.99, None), (104.0, 52.0, 16.0, 20.0, 0.95, None)]       # in the 200 x 136 photo; their ellipses do not meet
FACES_SMALL = [(40.0, 12.0, 30.0, 36.0, 0.99, None)]                                          # in the 128 x 64 photo
STEPS, STRENGTH, CFG = 5, 0.8, 4.0


@pytest.fixture(scope="module")
def rig(dev):
    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper
    from adaface_dev_amd.adaface.arc2face_models import clip_text_config
    from adaface_dev_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    cc = clip_text_config(hidden_size=128, num_attention_heads=2, num_hidden_layers=3, intermediate_size=512)
    ld = LatentDiffusion(_unet_cfg())
    ae = ld.instantiate_first_stage(dict(VAE_SMALL, double_z=True))
    with torch.no_grad():
        for n, p in ae.named_parameters():
            p.copy_(rng.synth_tensor(n, p.shape, seed=92))
    seen = []

    def detector(rgb):
        seen.append(rgb.shape)
        return FACES if rgb.shape[:2] == (136, 200) else FACES_SMALL

    w = AdaFaceWrapper(pipeline_name="inpaint", clip_config=cc, ldm=ld, vae=ae, device=dev, num_inference_steps=STEPS, face_detector=detector)
    rng.load_synth_weights(w.ldm.model.diffusion_model, seed=63)
    w = w.to(dev)
    pe = rng.synth_input("rep.pe", (1, 77, 128), seed=85).to(dev)
    ne = rng.synth_input("rep.ne", (1, 77, 128), seed=86).to(dev)
    return w, ae, pe, ne, seen


def _by_hand(dev, rig, photo, alpha, rect, work_hw, count, seed):
    """crop_resize_u8, inpaint_latents and sample_inpaint called as the wrapper calls them, then the fp64 paste-back of the decode."""
    from adaface_dev_amd import ops
    w, ae, pe, ne, _ = rig
    sampler = w._sampler()
    _, t_first = sampler.img2img_steps(STEPS, STRENGTH)
    gen = torch.Generator().manual_seed(seed)
    image, mask_lat = ops.crop_resize_u8(torch.from_numpy(photo).to(dev), alpha, rect, work_hw, THR)
    assert 0 < float(mask_lat.mean()) < 1
    x, z, n_fwd = w.ldm.inpaint_latents(image, count, t_first, generator=gen, first_stage_model=ae, from_noise=False)
    cond = (pe.repeat(count, 1, 1), [""] * count, {})
    uncond = (ne.repeat(count, 1, 1), [w.negative_prompt] * count, {})
    lat, _ = sampler.sample_inpaint(STEPS, STRENGTH, count, x, z, n_fwd, mask_lat, cond, guidance_scale=CFG,
                                    unconditional_conditioning=uncond, generator=gen)
    dec = ae.decode(lat / 0.18215).float().cpu().numpy()
    return R.paste_back_f64(dec, photo, alpha.cpu().numpy().astype(np.float64), rect)


def _check(out, photo, alpha, v64, count):
    """The photo's size; the photo's bytes outside the kernel's own alpha > 0 set; within one level of the fp64 paste-back."""
    H, W = photo.shape[:2]
    assert len(out) == count and all(im.size == (W, H) and im.mode == "RGB" for im in out)
    got = np.stack([np.asarray(im) for im in out])
    keep = alpha.cpu().numpy() == 0
    assert keep.any() and (~keep).any()
    for b in range(count):
        assert np.array_equal(got[b][keep], photo[keep])
    err = np.abs(got.astype(np.float64) - v64).max()
    print(f"wrapper repaint: max |out - v64| = {err:.4f} levels")
    assert err <= 1.0
    assert (got[:, ~keep] != photo[~keep]).any()
    return got


@pytest.mark.parametrize("scheduler", ["ddim", "dpm++"])
def test_wrapper_repaints_faces_in_a_crop(dev, rig, scheduler):
    """A 200 x 136 photo, two faces from a stub detector, work_size 64 x 64, crop_padding 0.5, two outputs."""
    from adaface_dev_amd import ops
    w, ae, pe, ne, seen = rig
    photo = _photo(136, 200, seed=17)
    w.default_scheduler_name = scheduler
    try:
        del seen[:]
        out = w(Image.fromarray(photo), None, prompt_embeds=(pe, ne), guidance_scale=CFG, out_image_count=2, ref_img_strength=STRENGTH,
                generator=torch.Generator().manual_seed(7), mask_image="face", crop_padding=0.5, work_size=(64, 64))
        assert seen == [(136, 200, 3)]
        e = R.face_ellipses(FACES, None, 1.3)
        rect = R.crop_region(R.ellipse_boxes(e), (136, 200), (64, 64), 0.5)
        assert rect[2] < 200 and rect[3] < 136                                    # a true crop: most of the photo never meets the VAE
        alpha = ops.face_alpha_mask(torch.from_numpy(e).to(dev), (136, 200), 0.25)
        _check(out, photo, alpha, _by_hand(dev, rig, photo, alpha, rect, (64, 64), 2, 7), 2)
    finally:
        w.default_scheduler_name = "ddim"


def test_wrapper_repaints_a_pil_mask_in_a_crop(dev, rig):
    """A PIL mask with crop_padding: the hard mask v >= 128 uploaded from the host, the region from its bounding box."""
    w, ae, pe, ne, seen = rig
    photo = _photo(136, 200, seed=18)
    m = np.zeros((136, 200), dtype=np.uint8)
    m[40:80, 80:120] = 255
    m[100:120, 10:40] = 100              # below 128: not repainted, not in the bounding box
    del seen[:]
    out = w(Image.fromarray(photo), None, prompt_embeds=(pe, ne), guidance_scale=CFG, out_image_count=2, ref_img_strength=STRENGTH,
            generator=torch.Generator().manual_seed(9), mask_image=Image.fromarray(m), crop_padding=0.5, work_size=(64, 64))
    assert seen == []                    # no detection for a caller's mask
    hard = m >= 128
    rect = R.crop_region(R.mask_bbox(hard), (136, 200), (64, 64), 0.5)
    assert rect == (60, 20, 80, 80)
    alpha = torch.from_numpy(hard.astype(np.float32)).to(dev)
    _check(out, photo, alpha, _by_hand(dev, rig, photo, alpha, rect, (64, 64), 2, 9), 2)


def test_wrapper_repaints_the_whole_photo(dev, rig):
    """crop_padding=None with "face": the rectangle is the whole 128 x 64 photo at its own size; the resample is the identity and the
    paste-back keeps the unmasked pixels exact."""
    from adaface_dev_amd import ops
    w, ae, pe, ne, seen = rig
    photo = _photo(64, 128, seed=19)
    out = w(Image.fromarray(photo), None, prompt_embeds=(pe, ne), guidance_scale=CFG, out_image_count=2, ref_img_strength=STRENGTH,
            generator=torch.Generator().manual_seed(11), mask_image="face")
    e = R.face_ellipses(FACES_SMALL, None, 1.3)
    alpha = ops.face_alpha_mask(torch.from_numpy(e).to(dev), (64, 128), 0.25)
    _check(out, photo, alpha, _by_hand(dev, rig, photo, alpha, (0, 0, 128, 64), (64, 128), 2, 11), 2)


def test_wrapper_face_index_repaints_one_face(dev, rig):
    """face_index=1: only the second face is repainted; every pixel of the first face's ellipse comes back unchanged."""
    from adaface_dev_amd import ops
    w, ae, pe, ne, seen = rig
    photo = _photo(136, 200, seed=20)
    out = w(photo, None, prompt_embeds=(pe, ne), guidance_scale=CFG, out_image_count=1, ref_img_strength=STRENGTH,
            generator=torch.Generator().manual_seed(13), mask_image="face", crop_padding=0.5, work_size=(64, 64), face_index=1)
    e1 = R.face_ellipses(FACES, 1, 1.3)
    alpha = ops.face_alpha_mask(torch.from_numpy(e1).to(dev), (136, 200), 0.25)
    rect = R.crop_region(R.ellipse_boxes(e1), (136, 200), (64, 64), 0.5)
    got = _check(out, photo, alpha, _by_hand(dev, rig, photo, alpha, rect, (64, 64), 1, 13), 1)
    first = R.alpha_mask_f64(R.face_ellipses(FACES, 0, 1.3), (136, 200), 0.0)[0] > 0
    assert first.sum() > 300 and np.array_equal(got[0][first], photo[first])
