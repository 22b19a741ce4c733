"""The Real-ESRGAN upscaler on a real MI355X (`pytest -m gpu`; INTEGRATION.md "Upscaling (Real-ESRGAN)"): RRDBNet.hip against the independent
restatement, the Upscaler's PIL round trip, and AdaFaceWrapper.forward(upscale=True).

The rule for the network: A is the restatement in fp64 (unrounded weights).  B is the same walk on the CPU with fp32 convolutions and every
tensor the device stores (the fp16 weights, the unshuffled input, each convolution's output after its fused epilogue) rounded to fp16;
e16 = max |255 B - 255 A| is what fp16 storage costs, in levels.  The device result must satisfy max |dev - rint(255 clamp(A))| <= 2 e16 + 1:
the factor 2 covers another summation order and fused epilogues, the 1 is the quantisation.

The weights are esrgan_restatement's gain = sqrt(2) networks, under which the image and the body dominate the output (e16 is 0.3-0.4 levels, a
zero image, a dropped body, a stale outer residual or dropped LeakyReLUs move the reference by 30-130 levels: tests/test_esrgan_host.py holds
that).  The gain = 0.1 weights run too, under the same rule, but are blind to everything in front of conv_hr and prove little."""
import numpy as np
import pytest
import torch

from esrgan_restatement import HE_GAIN, NETWORK_CASES, make_state_dict, network_case
from test_hip_face_repaint import _photo, rig                          # noqa: F401  (rig: the module fixture of the repaint tests)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.mark.parametrize("gain", [HE_GAIN, 0.1], ids=["he", "gain0.1"])
@pytest.mark.parametrize("scale,num_block,B,H,W", NETWORK_CASES, ids=["x4-2blocks", "x2-2blocks", "x4-6blocks"])
def test_rrdbnet_hip_vs_restatement(dev, scale, num_block, B, H, W, gain):
    """24 x 20: partial patches on both axes of the body and of every tail stage; 6 blocks: the buffer rotation over more than two RRDBs."""
    from adaface_dev_amd.adaface.esrgan import load_esrgan
    c = network_case(scale, num_block, B, H, W, gain)
    net = load_esrgan(c["sd"]).to(dev)
    got = net.hip(c["img"].to(dev))
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and got.shape == (B, H * scale, W * scale, 3) and got.is_cuda
    err = float((got.cpu().double() - c["want"]).abs().max())
    print(f"RRDBNet.hip x{scale} {num_block} blocks {B}x{H}x{W} gain {gain:.2f}: e16 {c['e16']:.4f} levels, device error {err:.1f} levels, "
          f"bound {2 * c['e16'] + 1:.2f}")
    assert err <= 2 * c["e16"] + 1, (err, c["e16"])
    assert torch.equal(net.hip(c["img"].to(dev)), got)                # the prepared weights are reused; the run is deterministic


def test_hip_follows_in_place_weight_edits(dev):
    """The prepared device weights are keyed on the parameters' versions: an in-place edit of one weight reaches the next hip() call."""
    from adaface_dev_amd.adaface.esrgan import load_esrgan
    c = network_case(*NETWORK_CASES[1])
    net = load_esrgan(c["sd"]).to(dev)
    img = c["img"].to(dev)
    before = net.hip(img)
    with torch.no_grad():
        net.conv_hr.weight.mul_(0.5)
    after = net.hip(img)
    assert float((after.float() - before.float()).abs().max()) > 10
    fresh = load_esrgan({k: v.detach().cpu() for k, v in net.state_dict().items()}).to(dev)
    assert torch.equal(fresh.hip(img), after)


def test_upscaler_pil_round_trip(dev):
    from PIL import Image
    from adaface_dev_amd.adaface.esrgan import Upscaler, load_esrgan
    c = network_case(*NETWORK_CASES[1])
    img = c["img"]
    up = Upscaler(load_esrgan(c["sd"]), device=dev)
    t = up(img)                                                       # a host tensor in, a host tensor out
    assert t.device.type == "cpu" and t.shape == (1, 48, 40, 3) and t.dtype == torch.uint8
    one = up(Image.fromarray(img[0].numpy()))
    assert isinstance(one, Image.Image) and one.size == (40, 48) and one.mode == "RGB"
    assert np.array_equal(np.asarray(one), t[0].numpy())
    many = up([Image.fromarray(img[0].numpy())] * 2)
    assert isinstance(many, list) and [m.size for m in many] == [(40, 48)] * 2 and np.array_equal(np.asarray(many[1]), t[0].numpy())
    d = up(img.to(dev))
    assert d.is_cuda and torch.equal(d.cpu(), t)
    assert float((t.double() - c["want"]).abs().max()) <= 2 * c["e16"] + 1       # the images that went in are the ones that came out upscaled


def test_wrapper_upscale(dev):
    """text2img with the small U-Net and VAE of the hires tests: upscale=True returns scale x the size and equals the Upscaler applied to the
    upscale=False images of the same seed; upscale=False with an upscaler loaded is bit-identical to the wrapper without one."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface.esrgan import load_esrgan
    from test_hip_hires import _small_wrapper
    w, _ = _small_wrapper(dev, 4)
    pe = rng.synth_input("hires.pe", (1, 77, 128), seed=85).to(dev)
    ne = rng.synth_input("hires.ne", (1, 77, 128), seed=86).to(dev)
    noise = rng.synth_input("hires.noise", (2, 4, 16, 16), seed=88).to(dev)
    run = lambda **kw: w(noise, None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=2, generator=torch.Generator().manual_seed(3), **kw)
    base = run()
    assert [im.size for im in base] == [(128, 128)] * 2
    up = w.load_upscaler(load_esrgan(make_state_dict(4, 1, seed=51, gain=HE_GAIN)))
    assert up.scale == 4
    off = run(upscale=False)
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(base, off))
    big = run(upscale=True)
    assert [im.size for im in big] == [(512, 512)] * 2 and all(im.mode == "RGB" for im in big)
    want = up(base)
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(big, want))
    # the upscaler's output follows its input (these weights are sensitive to it): the other image, or a shifted one, gives another result
    a0 = np.asarray(big[0]).astype(np.float64)
    assert np.abs(a0 - np.asarray(big[1])).max() > 20
    assert np.abs(a0 - np.asarray(up(base[0].transpose(0)))).max() > 20             # PIL transpose(0): left-right flip
    hi = run(upscale=True, hires_size=(128, 192), hires_strength=0.5, hires_steps=2)
    assert [im.size for im in hi] == [(512, 768)] * 2
    w.unload_upscaler()
    with pytest.raises(ValueError, match="no upscaler is loaded"):
        run(upscale=True)


def test_wrapper_upscales_the_repainted_photo(dev, rig):
    """The face-repaint path (the rig of tests/test_hip_face_repaint.py: a 200 x 136 photo, two faces from a stub detector, a 64 x 64 working
    crop): with upscale=True the pasted-back photos come back 2 x the photo's size and equal the Upscaler applied to the upscale=False result of
    the same seed."""
    from PIL import Image
    from adaface_dev_amd.adaface.esrgan import load_esrgan
    w, ae, pe, ne, seen = rig
    photo = Image.fromarray(_photo(136, 200, seed=17))
    run = lambda **kw: w(photo, None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=2, ref_img_strength=0.8,
                         generator=torch.Generator().manual_seed(7), mask_image="face", crop_padding=0.5, work_size=(64, 64), **kw)
    up = w.load_upscaler(load_esrgan(make_state_dict(2, 1, seed=52, gain=HE_GAIN)))
    try:
        plain = run()
        big = run(upscale=True)
    finally:
        w.unload_upscaler()
    assert [im.size for im in plain] == [(200, 136)] * 2 and [im.size for im in big] == [(400, 272)] * 2
    want = up(plain)
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(big, want))
    assert np.abs(np.asarray(big[0]).astype(np.float64) - np.asarray(big[1])).max() > 20       # two repaints, two upscaled photos
