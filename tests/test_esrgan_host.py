"""Real-ESRGAN host logic, CPU only (INTEGRATION.md "Upscaling (Real-ESRGAN)"): RRDBNet.forward against an independent restatement, the
published key layouts, the loader, the refusals of Upscaler and of AdaFaceWrapper.forward(upscale=True) before any GPU work, the call
sequence with upscale=False, and the bad-argument codes of the two C entry points (validation precedes any launch)."""
import os

import numpy as np
import pytest
import torch

from adaface_dev_amd import _lib
from adaface_dev_amd.adaface import esrgan
from adaface_dev_amd.adaface.esrgan import RRDBNet, Upscaler, load_esrgan
from esrgan_restatement import HE_GAIN, NETWORK_CASES, make_state_dict, network_case, quantise, rrdbnet_walk
from test_hires_host import _Recorder, _img, _spy_apply, _wrapper
from test_inpaint_host import _vae

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the network
@pytest.mark.parametrize("gain", [HE_GAIN, 0.1], ids=["he", "gain0.1"])
@pytest.mark.parametrize("scale", [4, 2, 1])
def test_forward_matches_the_restatement(scale, gain):
    """Both are fp32 walks of the same formulas through torch's conv2d: they differ by summation order inside the residual sums only.  1e-5 on
    outputs of magnitude <= 2 is ~50 fp32 roundings (the fp32 walk is 2e-6 from the fp64 one under the gain = sqrt(2) weights).  Those weights
    are the ones that see the body: test_network_references_are_sensitive."""
    sd = make_state_dict(scale, 2, seed=5 + scale, gain=gain)
    net = RRDBNet(scale=scale, num_block=2)
    net.load_state_dict(sd, strict=True)
    x = torch.rand(2, 3, 12, 8, generator=torch.Generator().manual_seed(scale))
    with torch.no_grad():
        got = net(x)
    ref = rrdbnet_walk(sd, x, scale, 2)
    assert got.shape == (2, 3, 12 * scale, 8 * scale) and got.dtype == torch.float32
    err = float((got - ref).abs().max())
    assert err <= 1e-5, err
    assert float(ref.std()) > 1e-3                                     # not a constant image


@pytest.mark.parametrize("case", NETWORK_CASES, ids=["x4-2blocks", "x2-2blocks", "x4-6blocks"])
def test_network_references_are_sensitive(case):
    """What the device tests (tests/test_hip_esrgan.py) and the forward test above can see.  Under the gain = sqrt(2) weights a zero image, a
    network without its body, an RRDB whose outer residual is the previous RRDB's input (a wrong buffer rotation) and dense blocks without
    their LeakyReLUs each move the quantised fp64 reference by at least five times the device bound 2 e16 + 1; and e16 is a real number.  Under
    the gain = 0.1 weights the same mutations stay inside that bound, which is why those weights alone would prove nothing."""
    scale, num_block = case[:2]
    c = network_case(*case)
    bound = 2 * c["e16"] + 1
    assert 0.1 < c["e16"] < 1.0, c["e16"]
    frac = float(((c["a"] < 0) | (c["a"] > 1)).double().mean())
    assert 0.02 < frac < 0.5 and float(c["a"].std()) > 0.2                          # spread over about [-0.1, 1.1], both clamps exercised
    moved = {"zero image": quantise(rrdbnet_walk(c["sd"], c["x"] * 0, scale, num_block))}
    for m in ("no_body", "stale_r2", "no_lrelu"):
        moved[m] = quantise(rrdbnet_walk(c["sd"], c["x"], scale, num_block, mutate=m))
    for name, q in moved.items():
        d = float((q - c["want"]).abs().max())
        print(f"x{scale} {num_block} blocks, {name}: reference moves by {d:.0f} levels, bound {bound:.2f}")
        assert d >= 5 * bound, (name, d, bound)
    # the fp32 forward test: the same mutations against its 1e-5
    f32 = rrdbnet_walk(c["sd"], c["x"].float(), scale, num_block)
    for m in ("no_body", "stale_r2", "no_lrelu"):
        assert float((rrdbnet_walk(c["sd"], c["x"].float(), scale, num_block, mutate=m) - f32).abs().max()) > 1e-2
    blind = network_case(*case, gain=0.1)
    d = float((quantise(rrdbnet_walk(blind["sd"], blind["x"], scale, num_block, mutate="no_body")) - blind["want"]).abs().max())
    assert d <= 2 * blind["e16"] + 1


def published_layout(in_ch, num_block):
    """RealESRGAN_x4plus (3, 23), RealESRGAN_x2plus (12, 23), RealESRGAN_x4plus_anime_6B (3, 6): name -> shape, written out."""
    lay = {"conv_first.weight": (64, in_ch, 3, 3), "conv_first.bias": (64,)}
    for i in range(num_block):
        for rdb in ("rdb1", "rdb2", "rdb3"):
            for conv, (co, ci) in (("conv1", (32, 64)), ("conv2", (32, 96)), ("conv3", (32, 128)), ("conv4", (32, 160)), ("conv5", (64, 192))):
                lay[f"body.{i}.{rdb}.{conv}.weight"] = (co, ci, 3, 3)
                lay[f"body.{i}.{rdb}.{conv}.bias"] = (co,)
    for name in ("conv_body", "conv_up1", "conv_up2", "conv_hr"):
        lay[name + ".weight"], lay[name + ".bias"] = (64, 64, 3, 3), (64,)
    lay["conv_last.weight"], lay["conv_last.bias"] = (3, 64, 3, 3), (3,)
    return lay


@pytest.mark.parametrize("scale,in_ch,num_block", [(4, 3, 23), (2, 12, 23), (4, 3, 6)])
def test_key_names_and_shapes_match_the_published_layouts(scale, in_ch, num_block):
    lay = published_layout(in_ch, num_block)
    assert len(lay) == 2 * (6 + 15 * num_block)
    sd = RRDBNet(scale=scale, num_block=num_block).state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == lay
    assert esrgan.expected_keys(scale, num_block) == lay
    # a few entries and the totals, literally (RealESRGAN_x4plus.pth holds 702 tensors and 16,697,987 parameters)
    assert len(sd) == {23: 702, 6: 192}[num_block]
    last = num_block - 1
    assert tuple(sd[f"body.{last}.rdb3.conv5.weight"].shape) == (64, 192, 3, 3) and tuple(sd[f"body.{last}.rdb3.conv5.bias"].shape) == (64,)
    assert tuple(sd["body.0.rdb1.conv1.weight"].shape) == (32, 64, 3, 3) and tuple(sd["body.3.rdb2.conv4.weight"].shape) == (32, 160, 3, 3)
    assert tuple(sd["conv_first.weight"].shape) == (64, in_ch, 3, 3) and tuple(sd["conv_last.weight"].shape) == (3, 64, 3, 3)
    assert f"body.{num_block}.rdb1.conv1.weight" not in sd
    if (scale, num_block) == (4, 23):
        assert sum(v.numel() for v in sd.values()) == 16697987


# ---------------------------------------------------------------------------------------------------------------- the loader
def test_loader_infers_scale_and_blocks_and_unwraps(tmp_path):
    for scale, nb in ((4, 2), (2, 3), (1, 1)):
        sd = make_state_dict(scale, nb, seed=3)
        net = load_esrgan(sd)
        assert (net.scale, len(net.body)) == (scale, nb) and not net.training
        for k, v in net.state_dict().items():
            assert torch.equal(v, sd[k]), k
    sd = make_state_dict(4, 1, seed=4)
    other = make_state_dict(4, 2, seed=9)
    assert len(load_esrgan({"params": other, "params_ema": sd}).body) == 1          # params_ema wins
    assert len(load_esrgan({"params": other}).body) == 2
    path = tmp_path / "net.pth"
    torch.save({"params_ema": {k: v.half() for k, v in sd.items()}}, path)
    net = load_esrgan(str(path))
    assert net.conv_first.weight.dtype == torch.float32
    assert torch.equal(net.conv_last.weight, sd["conv_last.weight"].half().float())


def test_loader_refusals_name_the_key():
    sd = make_state_dict(4, 2, seed=3)
    miss = {k: v for k, v in sd.items() if k != "body.1.rdb2.conv3.bias"}
    with pytest.raises(ValueError, match=r"missing keys: body\.1\.rdb2\.conv3\.bias"):
        load_esrgan(miss)
    with pytest.raises(ValueError, match=r"missing keys: body\.0\.rdb1\.conv1\.bias, body\.0\.rdb1\.conv1\.weight"):   # a hole in the numbering
        load_esrgan({k: v for k, v in sd.items() if not k.startswith("body.0.")})
    with pytest.raises(ValueError, match=r"unexpected keys: conv_extra\.weight"):
        load_esrgan(dict(sd, **{"conv_extra.weight": torch.zeros(1)}))
    bad = dict(sd)
    bad["conv_hr.weight"] = torch.zeros(64, 32, 3, 3)
    with pytest.raises(ValueError, match=r"mis-shaped keys: conv_hr\.weight \(64, 32, 3, 3\)"):
        load_esrgan(bad)
    with pytest.raises(ValueError, match=r"conv_first\.weight"):
        load_esrgan({k: v for k, v in sd.items() if k != "conv_first.weight"})
    with pytest.raises(ValueError, match=r"conv_first\.weight takes 5 channels"):
        load_esrgan(dict(sd, **{"conv_first.weight": torch.zeros(64, 5, 3, 3)}))
    with pytest.raises(ValueError, match="width 64 with growth 32"):
        load_esrgan(dict(sd, **{"conv_first.weight": torch.zeros(32, 3, 3, 3)}))
    with pytest.raises(ValueError, match="width 64 with growth 32"):
        load_esrgan(dict(sd, **{"body.0.rdb1.conv1.weight": torch.zeros(16, 64, 3, 3)}))
    with pytest.raises(ValueError, match=r"missing keys: body\.0\.rdb1\.conv1\.weight"):     # SRVGGNet-like: no body at all
        load_esrgan({k: v for k, v in sd.items() if not k.startswith("body.")})


# ---------------------------------------------------------------------------------------------------------------- Upscaler
class _NoHip(RRDBNet):
    def hip(self, images_u8):
        raise AssertionError("the device path was reached")


def _upscaler(scale=4):
    net = _NoHip(scale=scale, num_block=1)
    net.to = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the network was moved to the device"))
    return Upscaler(net)


def test_upscaler_refuses_before_any_gpu_work():
    from PIL import Image
    up = _upscaler(2)
    assert up.scale == 2
    for shape in ((1, 7, 8, 3), (1, 8, 9, 3)):
        with pytest.raises(ValueError, match="multiples of 2"):
            up(torch.zeros(shape, dtype=torch.uint8))
    with pytest.raises(ValueError, match="at most 1024"):
        up(torch.zeros((1, 8, 1026, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="at most 1024"):
        up(Image.new("RGB", (1028, 16)))
    with pytest.raises(ValueError, match="multiples of 2"):
        up([Image.new("RGB", (15, 16))])
    with pytest.raises(ValueError, match="one size"):
        up([Image.new("RGB", (16, 16)), Image.new("RGB", (16, 18))])
    for bad in (torch.zeros((1, 8, 8, 3)), torch.zeros((8, 8, 3), dtype=torch.uint8), torch.zeros((1, 8, 8, 4), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="uint8 tensor"):
            up(bad)
    for bad in ([], "photo.png", [np.zeros((8, 8, 3), dtype=np.uint8)]):
        with pytest.raises(ValueError, match="PIL"):
            up(bad)
    with pytest.raises(ValueError, match="multiples of 4"):
        _upscaler(1)(torch.zeros((1, 8, 10, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="RRDBNet"):
        Upscaler(torch.nn.Conv2d(3, 3, 3))
    with pytest.raises(ValueError, match="width 64"):
        Upscaler(RRDBNet(num_block=1, num_feat=32))


# ---------------------------------------------------------------------------------------------------------------- wrapper
def test_wrapper_loads_and_unloads_an_upscaler(tmp_path):
    up = _upscaler()
    w = _wrapper(upscaler=up)
    assert w.upscaler is up and "upscaler" not in dict(w.named_modules())
    w.unload_upscaler()
    assert w.upscaler is None
    net = RRDBNet(num_block=1)
    assert w.load_upscaler(net).net is net and w.upscaler.scale == 4
    sd = make_state_dict(2, 1, seed=2)
    assert w.load_upscaler(sd).scale == 2
    path = tmp_path / "x2.pth"
    torch.save({"params": sd}, path)
    assert w.load_upscaler(str(path)).scale == 2
    with pytest.raises(ValueError, match="conv_first.weight"):
        w.load_upscaler({"body.weight": torch.zeros(1)})


def _no_detector(rgb):
    raise AssertionError("the detector must not run before the refusals")


def test_wrapper_upscale_refuses_before_any_gpu_work():
    from PIL import Image
    pe = torch.zeros(1, 77, 64)
    noise = torch.zeros(1, 4, 16, 8)
    # no upscaler loaded
    w = _wrapper(vae=_vae())
    calls = _spy_apply(w)
    with pytest.raises(ValueError, match="no upscaler is loaded"):
        w(noise, None, prompt_embeds=(pe, pe), out_image_count=1, upscale=True)
    # no vae: latents come back
    w = _wrapper(upscaler=_upscaler())
    calls += _spy_apply(w)
    with pytest.raises(ValueError, match="needs a vae"):
        w(noise, None, prompt_embeds=(pe, pe), out_image_count=1, upscale=True)
    # a result over the upscaler's input limit: text2img, hires_size, img2img, inpaint, the repaint path
    up = _upscaler()
    up.max_input_side = 96
    w = _wrapper(vae=_vae(), upscaler=up)
    calls += _spy_apply(w)
    with pytest.raises(ValueError, match="at most 96"):
        w(noise, None, prompt_embeds=(pe, pe), out_image_count=1, upscale=True)             # 64 x 128 pixels
    with pytest.raises(ValueError, match="at most 96"):
        w(torch.zeros(1, 4, 8, 8), None, prompt_embeds=(pe, pe), out_image_count=1, hires_size=(128, 64), upscale=True)
    big = Image.new("RGB", (128, 64))
    for name in ("img2img", "inpaint"):
        wi = _wrapper(name, vae=_vae(), upscaler=up)
        calls += _spy_apply(wi)
        wi.vae.encode_q_sample = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the encoder was reached"))
        kw = {"mask_image": Image.new("L", (128, 64), 255)} if name == "inpaint" else {}
        with pytest.raises(ValueError, match="at most 96"):
            wi(big, None, prompt_embeds=(pe, pe), out_image_count=1, upscale=True, **kw)
    wi.face_detector = _no_detector
    with pytest.raises(ValueError, match="at most 96"):
        wi(np.zeros((50, 130, 3), dtype=np.uint8), None, prompt_embeds=(pe, pe), out_image_count=1, mask_image="face", crop_padding=0.5,
           upscale=True)
    up2 = _upscaler(2)
    wi.load_upscaler(up2)
    with pytest.raises(ValueError, match="multiples of 2"):                               # a photo of any size comes back: odd sides
        wi(np.zeros((51, 70, 3), dtype=np.uint8), None, prompt_embeds=(pe, pe), out_image_count=1, mask_image="face", crop_padding=0.5,
           upscale=True)
    assert calls == []


def test_forward_with_upscale_false_is_unchanged():
    """upscale=False, with or without an upscaler loaded: one sampler.sample call with the arguments forward has always passed, the upscaler never
    touched, the latents returned (no vae here, as in test_hires_host)."""
    pe, ne = torch.zeros(1, 77, 64), torch.ones(1, 77, 64)
    noise = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(0))
    g = torch.Generator().manual_seed(1)

    class _Spy:
        scale = 4

        def __getattr__(self, name):
            raise AssertionError(f"the upscaler was touched ({name})")

    for extra in ({}, dict(upscale=False)):
        for up in (None, _Spy()):
            w = _wrapper(num_inference_steps=10)
            w.__dict__["upscaler"] = up
            log = []
            w._sampler = lambda: _Recorder(w.ldm, log)
            out = w(noise, "p", prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=2, generator=g, **extra)
            assert len(log) == 1
            name, S, B, shape, kw = log[0]
            assert (name, S, B, shape) == ("sample", 10, 2, (4, 8, 8))
            assert sorted(kw) == ["conditioning", "generator", "guidance_scale", "unconditional_conditioning", "verbose", "x_T"]
            assert torch.equal(kw["x_T"], noise) and kw["generator"] is g and kw["guidance_scale"] == 4.0
            assert torch.equal(out, noise + 1.0)


def test_to_pil_sends_quantised_images_through_the_upscaler_on_request():
    """_to_pil(latents, upscale): the uint8 NHWC tensor goes to Upscaler.upscale_u8 only under upscale=True, and what comes back becomes the PIL
    images; without it the images are the quantised decode as before."""
    import types
    w = _wrapper()
    dec = torch.rand(2, 3, 16, 24, generator=torch.Generator().manual_seed(3)) * 2.4 - 1.2
    w.vae = types.SimpleNamespace(decode=lambda z: dec)
    seen = []

    def upscale_u8(t):
        seen.append(t)
        return t.repeat_interleave(2, 1).repeat_interleave(2, 2)

    w.__dict__["upscaler"] = types.SimpleNamespace(upscale_u8=upscale_u8)
    lat = torch.zeros(2, 4, 2, 3)
    want = ((dec / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).numpy()
    plain = w._to_pil(lat)
    assert seen == [] and all(np.array_equal(np.asarray(p), q) for p, q in zip(plain, want))
    big = w._to_pil(lat, True)
    assert len(seen) == 1 and seen[0].dtype == torch.uint8 and seen[0].is_contiguous() and np.array_equal(seen[0].numpy(), want)
    assert [im.size for im in big] == [(48, 32)] * 2
    assert np.array_equal(np.asarray(big[1]), want[1].repeat(2, 0).repeat(2, 1))


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_header_and_exports_carry_the_kernels():
    with open(os.path.join(ROOT, "include", "adaface_hip.h")) as f:
        header = f.read()
    assert "int af_dense_conv3x3(const void* x, int ldx, int cin, const void* wt, const void* bias, void* out, int ldo, int cout," in header
    assert "int af_u8_unshuffle_f16(const void* img_u8, void* out, int B, int H, int W, int r, int cpad, void* stream);" in header
    assert "af_dense_conv3x3" in _lib.EXPORTS and "af_u8_unshuffle_f16" in _lib.EXPORTS


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """No GPU here: every call below must come back AF_E_BADARG from the argument checks (a launch would fail differently).  Pointers are
    made-up aligned addresses that are never dereferenced."""
    L = _lib.lib()
    P = 1 << 20
    good = dict(x=P, ldx=192, cin=96, wt=2 * P, bias=None, out=P + 2 * 96, ldo=192, cout=32, r1=None, ldr1=0, alpha=1.0, r2=None, ldr2=0,
                beta=1.0, slope=0.2, upsample=0, out_mode=0, B=2, H=19, W=21)

    def call(**kw):
        a = dict(good, **kw)
        return L.af_dense_conv3x3(a["x"], a["ldx"], a["cin"], a["wt"], a["bias"], a["out"], a["ldo"], a["cout"], a["r1"], a["ldr1"], a["alpha"],
                                  a["r2"], a["ldr2"], a["beta"], a["slope"], a["upsample"], a["out_mode"], a["B"], a["H"], a["W"], None)

    far = 1 << 40
    cases = [dict(x=None), dict(wt=None), dict(out=None), dict(cin=48), dict(cin=224), dict(cin=0), dict(cout=65), dict(cout=0),
             dict(ldx=64), dict(ldx=100), dict(ldo=24, out=far), dict(ldo=36, out=far), dict(out=P + 2 * 64), dict(out=P + 2 * 168),
             dict(out=P), dict(out=P + 2 * 96, ldo=200), dict(out=P + 2 * 96, upsample=1), dict(r2=far, ldr2=64),
             dict(r1=far, ldr1=16), dict(r1=far, ldr1=36),
             # r1 / r2 inside out's byte range must be exactly the out elements or other channels of the same rows
             dict(r1=P + 2 * 96 + 2 * 16, ldr1=192), dict(r1=P + 2 * 96 + 2 * 192, ldr1=192), dict(r1=P + 2 * 96, ldr1=96),
             dict(r1=far, ldr1=64, r2=P + 2 * 96 - 2 * 8, ldr2=192), dict(x=P + 2), dict(wt=2 * P + 8), dict(r1=far + 4, ldr1=64),
             dict(upsample=2), dict(out_mode=2), dict(B=0), dict(H=0), dict(W=-1),
             dict(out=far, B=16, H=1024, W=1024),                                             # B*H*W*ldx = 2^31 * 1.5
             dict(x=far, ldx=64, cin=64, cout=32, out=3 * far, out_mode=1, upsample=1, B=1, H=4096, W=4096)]   # B*Ho*Wo*cout = 2^31
    for kw in cases:
        assert call(**kw) == _lib.AF_E_BADARG, kw
        assert b"af_dense_conv3x3" in L.af_last_error()
    assert call(out=P + 2 * 64) == _lib.AF_E_BADARG and b"overlaps the input channels" in L.af_last_error()
    assert call(r2=far, ldr2=64) == _lib.AF_E_BADARG and b"r2 needs r1" in L.af_last_error()
    assert call(r1=P + 2 * 96 + 2 * 16, ldr1=192) == _lib.AF_E_BADARG and b"r1 overlaps out" in L.af_last_error()

    def unshuffle(img=P, out=2 * P, B=2, H=8, W=12, r=2, cpad=32):
        return L.af_u8_unshuffle_f16(img, out, B, H, W, r, cpad, None)

    for kw in (dict(img=None), dict(out=None), dict(r=3), dict(r=0), dict(H=7), dict(W=10, r=4), dict(cpad=16), dict(cpad=48), dict(r=4, cpad=32),
               dict(out=2 * P + 8), dict(B=0), dict(B=1024, H=1024, W=1024, r=1)):
        assert unshuffle(**kw) == _lib.AF_E_BADARG, kw
        assert b"af_u8_unshuffle_f16" in L.af_last_error()
