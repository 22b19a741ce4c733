"""GFPGAN face restoration on a real MI355X (`pytest -m gpu`; INTEGRATION.md "Face restoration (GFPGAN)"): GFPGANv1Clean.hip against the
independent restatement, FaceRestorer with a stub detector, and AdaFaceWrapper.forward(restore_faces=True).

The rule for the network, in levels of 127.5 (the output is nominally in [-1, 1]): A is the restatement in fp64.  B is the same walk on the CPU
in fp32 with every tensor the device stores rounded to fp16 (the plain weights, the per-sample modulated weights, every convolution and
epilogue output, the resampled maps, the latents); e16 = 127.5 max |B - A| is what fp16 storage costs.  The device must satisfy
127.5 max |dev - A| <= 2 e16: the factor 2 is the margin the project grants another summation order and fused epilogues.

Measured on the MI355X (profiles/gfpgan.txt): 32-pixel network e16 0.469, device 0.529; 64-pixel network e16 0.705, device 0.757.

The weights are gfpgan_restatement's, under which every branch matters (tests/test_gfpgan_host.py holds that each of seven wrong networks moves
A by more than 100 times the bound)."""
import numpy as np
import pytest
import torch

from gfpgan_restatement import CFG32, LEVELS, make_state_dict, network_case
from test_hip_face_repaint import _photo, rig                          # noqa: F401  (rig: the module fixture of the repaint tests)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _crops(x, dev):
    """fp64 NCHW [B, 3, S, S] of fp16-representable values -> what ops.face_align_crop_any writes: fp16 NHWC [B, S, S, 8], zeros behind RGB."""
    B, _, S, _ = x.shape
    c = torch.zeros((B, S, S, 8), dtype=torch.float16)
    c[..., :3] = x.permute(0, 2, 3, 1).half()
    return c.to(dev)


@pytest.mark.parametrize("name", ["32", "64"])
def test_gfpgan_hip_vs_restatement(dev, name):
    """B = 2 with different inputs: per-sample weights, one convolution launch per sample.  32: widths 32 / 64, three levels; 64: 64 / 128,
    four levels, the first whose channel_multiplier shows."""
    from adaface_dev_amd.adaface.gfpgan import load_gfpgan
    c = network_case(name)
    S = c["cfg"]["out_size"]
    net = load_gfpgan(c["sd"]).to(dev)
    crops = _crops(c["x"], dev)
    got = net.hip(crops)
    torch.cuda.synchronize()
    assert got.dtype == torch.float16 and got.shape == (2, S, S, 8) and got.is_cuda and got.is_contiguous()
    assert not got[..., 3:].view(torch.int16).any()                                   # zeros behind RGB
    err = LEVELS * float((got[..., :3].cpu().double().permute(0, 3, 1, 2) - c["a"]).abs().max())
    print(f"GFPGANv1Clean.hip {name}: e16 {c['e16']:.4f} levels, device error {err:.4f} levels, bound {2 * c['e16']:.4f}")
    assert err <= 2 * c["e16"], (err, c["e16"])
    assert torch.equal(net.hip(crops), got)                                           # prepared weights and scratch are reused; the run is deterministic
    one = net.hip(crops[1:])                                                          # sample 1 alone: its own weights, not sample 0's
    assert LEVELS * float((one[0, ..., :3].cpu().double().permute(2, 0, 1) - c["a"][1]).abs().max()) <= 2 * c["e16"]


def test_hip_follows_in_place_weight_edits(dev):
    """The prepared device weights are keyed on the parameters' and buffers' versions: an in-place edit of a modulated weight, of a noise
    weight or of a noise map reaches the next hip() call."""
    from adaface_dev_amd.adaface.gfpgan import load_gfpgan
    c = network_case("32")
    net = load_gfpgan(c["sd"]).to(dev)
    crops = _crops(c["x"], dev)
    before = net.hip(crops).clone()
    with torch.no_grad():
        net.stylegan_decoder.to_rgbs[2].modulated_conv.weight.mul_(0.5)
    after = net.hip(crops).clone()
    assert LEVELS * float((after.float() - before.float()).abs().max()) > 10
    with torch.no_grad():
        net.stylegan_decoder.noises.noise6.mul_(-1.0)
    flipped = net.hip(crops).clone()
    assert LEVELS * float((flipped.float() - after.float()).abs().max()) > 10
    fresh = load_gfpgan({k: v.detach().cpu() for k, v in net.state_dict().items()}).to(dev)
    assert torch.equal(fresh.hip(crops), flipped)


# ---------------------------------------------------------------------------------------------------------------- FaceRestorer
def _kps(scale, theta, tx, ty, size=32):
    """Landmarks that are the image of the size-pixel template under a similarity: the fitted crop -> image matrix is that similarity."""
    from adaface_dev_amd.adaface.gfpgan import ffhq_template
    c, s = scale * np.cos(theta), scale * np.sin(theta)
    return (ffhq_template(size) @ np.array([[c, -s], [s, c]]).T + [tx, ty]).tolist()


def _footprint(fr, rgb):
    """Pixels some crop can change: m > erode for a face, in fp64 from the restorer's own matrices, with a margin of 1e-3 pixel."""
    fwd, _ = fr.face_matrices(rgb)
    H, W = rgb.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    S = fr.size
    inside = np.zeros((H, W), dtype=bool)
    for M in fwd.astype(np.float64):
        u, v = M[0, 0] * xs + M[0, 1] * ys + M[0, 2], M[1, 0] * xs + M[1, 1] * ys + M[1, 2]
        inside |= np.minimum(np.minimum(u, v), np.minimum(S - 1 - u, S - 1 - v)) > fr.erode * S - 1e-3
    return inside


def test_face_restorer_with_a_stub_detector(dev):
    """A 96 x 120 photo, two faces (fixed landmarks): the call equals restore_u8, the PIL round trip works, pixels outside every crop are
    bit-identical and pixels inside change, the restored crops are what the network gives for the aligned crops, and an image without a face
    comes back as it went in."""
    from PIL import Image
    from adaface_dev_amd import ops
    from adaface_dev_amd.adaface.gfpgan import FaceRestorer, load_gfpgan
    faces = [(20.0, 10.0, 40.0, 50.0, 0.99, _kps(1.4, 0.15, 18.0, 12.0)), (70.0, 40.0, 40.0, 50.0, 0.9, _kps(1.2, -0.25, 66.0, 52.0))]
    seen = []
    fr = FaceRestorer(load_gfpgan(network_case("32")["sd"]), lambda rgb: seen.append(rgb.shape) or faces, device=dev)
    photo = _photo(96, 120, seed=31)
    tp = torch.from_numpy(photo)
    out = fr.restore_u8(tp)
    assert out.is_cuda and out.dtype == torch.uint8 and out.shape == (96, 120, 3) and seen == [(96, 120, 3)]
    got = out.cpu().numpy()
    inside = _footprint(fr, photo)
    assert inside.any() and (~inside).any()
    assert np.array_equal(got[~inside], photo[~inside])
    assert (got[inside] != photo[inside]).mean() > 0.5
    # by hand: align, restore, paste
    fwd, inv = fr.face_matrices(photo)
    crops = ops.face_align_crop_any(tp.to(dev), torch.from_numpy(inv).to(dev), 32)
    want = ops.face_paste_affine_u8(tp.to(dev), fr.net.hip(crops), torch.from_numpy(fwd).to(dev), 0.05 * 32, 0.10 * 32)
    assert torch.equal(want, out)
    # the kinds that go in come out
    assert torch.equal(fr(tp), out.cpu()) and fr(tp).device.type == "cpu" and torch.equal(fr(tp.to(dev)), out)
    pil = fr(Image.fromarray(photo))
    assert isinstance(pil, Image.Image) and pil.size == (120, 96) and np.array_equal(np.asarray(pil), got)
    arr = fr([photo, Image.fromarray(photo)])
    assert isinstance(arr[0], np.ndarray) and np.array_equal(arr[0], got) and np.array_equal(np.asarray(arr[1]), got)
    # no face: the input
    none = FaceRestorer(fr.net, lambda rgb: [], device=dev)
    assert torch.equal(none.restore_u8(tp).cpu(), tp) and np.array_equal(np.asarray(none(Image.fromarray(photo))), photo)


# ---------------------------------------------------------------------------------------------------------------- wrapper
def test_wrapper_restores_faces_before_upscaling(dev):
    """text2img with the small U-Net and VAE of the hires tests (128 x 128 images), a stub detector and the 32-pixel network:
    restore_faces=True equals the FaceRestorer applied to the restore_faces=False images of the same seed and differs from them only inside the
    crops; restore_faces=False with a restorer loaded is the wrapper without one; with upscale=True the restored image is what gets
    upscaled."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface.esrgan import load_esrgan
    from esrgan_restatement import HE_GAIN
    from esrgan_restatement import make_state_dict as esrgan_state_dict
    from test_hip_hires import _small_wrapper
    w, _ = _small_wrapper(dev, 4)
    pe = rng.synth_input("hires.pe", (1, 77, 128), seed=85).to(dev)
    ne = rng.synth_input("hires.ne", (1, 77, 128), seed=86).to(dev)
    noise = rng.synth_input("hires.noise", (2, 4, 16, 16), seed=88).to(dev)
    run = lambda **kw: w(noise, None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=2, generator=torch.Generator().manual_seed(3), **kw)
    base = run()
    with pytest.raises(ValueError, match="no face restorer is loaded"):
        run(restore_faces=True)
    faces = [(30.0, 20.0, 60.0, 70.0, 0.99, _kps(2.1, 0.1, 28.0, 22.0))]
    fr = w.load_face_restorer(make_state_dict(CFG32, seed=102), detect_faces=lambda rgb: faces)
    off = run(restore_faces=False)
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(base, off))
    rest = run(restore_faces=True)
    assert [im.size for im in rest] == [(128, 128)] * 2 and all(im.mode == "RGB" for im in rest)
    want = fr(base)
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(rest, want))
    inside = _footprint(fr, np.asarray(base[0]))
    assert inside.any() and (~inside).any()
    for a, b in zip(rest, base):
        a, b = np.asarray(a), np.asarray(b)
        assert np.array_equal(a[~inside], b[~inside]) and (a[inside] != b[inside]).mean() > 0.5
    up = w.load_upscaler(load_esrgan(esrgan_state_dict(4, 1, seed=51, gain=HE_GAIN)))
    big = run(restore_faces=True, upscale=True)
    assert [im.size for im in big] == [(512, 512)] * 2
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(big, up(rest)))
    assert any(not np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(big, up(base)))
    w.unload_upscaler()
    w.unload_face_restorer()
    with pytest.raises(ValueError, match="no face restorer is loaded"):
        run(restore_faces=True)


def test_wrapper_restores_the_repainted_photo(dev, rig):
    """The face-repaint path (the rig of tests/test_hip_face_repaint.py: a 200 x 136 photo, a 64 x 64 working crop): with restore_faces=True the
    pasted-back photos equal the FaceRestorer applied to the restore_faces=False result of the same seed."""
    from PIL import Image
    w, ae, pe, ne, seen = rig
    photo = Image.fromarray(_photo(136, 200, seed=17))
    run = lambda **kw: w(photo, None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=2, ref_img_strength=0.8,
                         generator=torch.Generator().manual_seed(7), mask_image="face", crop_padding=0.5, work_size=(64, 64), **kw)
    faces = [(60.0, 30.0, 40.0, 50.0, 0.99, _kps(1.6, -0.1, 58.0, 28.0))]
    fr = w.load_face_restorer(make_state_dict(CFG32, seed=103), detect_faces=lambda rgb: faces)
    try:
        plain = run()
        rest = run(restore_faces=True)
    finally:
        w.unload_face_restorer()
    assert [im.size for im in rest] == [(200, 136)] * 2
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(rest, fr(plain)))
    assert all(not np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(rest, plain))
