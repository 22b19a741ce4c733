"""GFPGAN face restoration on the CPU (INTEGRATION.md "Face restoration (GFPGAN)"): the published key layout, the strict loader, the plain-torch
forward against the independent restatement in fp64, what the network-level references can see, the host side of FaceRestorer, the refusal of
AdaFaceWrapper.forward(restore_faces=True) before any GPU work, and the bad-argument codes of the new C entry points (validation precedes any
launch)."""
import os
import types

import numpy as np
import pytest
import torch

from adaface_dev_amd import _lib
from adaface_dev_amd.adaface import gfpgan
from adaface_dev_amd.adaface.face_align import estimate_similarity
from adaface_dev_amd.adaface.gfpgan import FFHQ_TEMPLATE_512, FaceRestorer, GFPGANv1Clean, expected_keys, ffhq_template, load_gfpgan
from gfpgan_restatement import CFG32, CFG64, LEVELS, MUTATIONS, gfpgan_walk, key_shapes, make_state_dict, network_case
from test_hires_host import _spy_apply, _wrapper
from test_inpaint_host import _vae

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- layout and loader
def test_v14_configuration_has_285_keys_and_87m_parameters():
    with torch.device("meta"):
        net = GFPGANv1Clean(out_size=512, num_style_feat=512, channel_multiplier=2, num_mlp=8, narrow=1)
    sd = net.state_dict()
    assert len(sd) == 285
    assert round(sum(v.numel() for v in sd.values()) / 1e6, 1) == 87.1
    want = expected_keys()
    assert {k: tuple(v.shape) for k, v in sd.items()} == want == key_shapes(dict(out_size=512, num_style_feat=512, channel_multiplier=2, narrow=1))
    assert want["stylegan_decoder.style_convs.13.modulated_conv.weight"] == (1, 64, 64, 3, 3)
    assert want["final_linear.weight"] == (16 * 512, 256 * 16) and want["condition_shift.6.2.weight"] == (32, 32, 3, 3)
    assert want["stylegan_decoder.noises.noise14"] == (1, 1, 512, 512) and want["conv_body_first.weight"] == (32, 3, 1, 1)


@pytest.mark.parametrize("cfg", [CFG32, CFG64], ids=["32", "64"])
def test_small_configurations_match_the_restatements_layout(cfg):
    assert expected_keys(**cfg) == key_shapes(cfg)
    assert {k: tuple(v.shape) for k, v in GFPGANv1Clean(num_mlp=8, **cfg).state_dict().items()} == key_shapes(cfg)


@pytest.mark.parametrize("wrap", [None, "params_ema", "params"])
def test_loader_is_strict_under_every_wrapper(wrap, tmp_path):
    sd = make_state_dict(CFG32, seed=3)
    box = (lambda d: d) if wrap is None else (lambda d: {wrap: d})
    net = load_gfpgan(box(sd))
    assert (net.out_size, net.num_style_feat, net.narrow) == (32, 64, 0.125) and not net.training
    assert all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())
    path = tmp_path / "g.pth"
    torch.save(box(sd), path)
    assert torch.equal(load_gfpgan(str(path)).final_linear.bias, sd["final_linear.bias"])
    miss = {k: v for k, v in sd.items() if k != "condition_shift.1.2.bias"}
    with pytest.raises(ValueError, match=r"missing keys: condition_shift\.1\.2\.bias"):
        load_gfpgan(box(miss))
    with pytest.raises(ValueError, match=r"unexpected keys: stylegan_decoder\.style_conv1\.activate\.bias"):
        load_gfpgan(box(dict(sd, **{"stylegan_decoder.style_conv1.activate.bias": torch.zeros(64)})))
    with pytest.raises(ValueError, match=r"mis-shaped keys: toRGB\.0\.weight \(3, 32, 3, 3\)"):
        load_gfpgan(box(dict(sd, **{"toRGB.0.weight": torch.zeros(3, 32, 3, 3)})))


def test_loader_infers_the_configuration_and_refuses_other_layouts():
    net = load_gfpgan(make_state_dict(CFG64, seed=4))
    assert (net.out_size, net.num_style_feat, net.channel_multiplier, net.narrow) == (64, 64, 2, 0.25)
    sd = make_state_dict(CFG32, seed=3)
    with pytest.raises(ValueError, match="different_w=False"):
        load_gfpgan(dict(sd, **{"final_linear.weight": torch.zeros(64, 512)}))
    with pytest.raises(ValueError, match="sft_half=False"):
        load_gfpgan(dict(sd, **{"condition_scale.0.2.weight": torch.zeros(64, 32, 3, 3)}))
    v1 = {k.replace("conv_body_first.", "conv_body_first.0."): v for k, v in sd.items()}
    with pytest.raises(ValueError, match="non-clean architecture"):
        load_gfpgan(v1)
    with pytest.raises(ValueError, match="missing key conv_body_first.weight"):
        load_gfpgan({"conv_first.weight": torch.zeros(64, 3, 3, 3)})


# ---------------------------------------------------------------------------------------------------------------- the network
@pytest.mark.parametrize("name", ["32", "64"])
def test_forward_matches_the_restatement_in_fp64(name):
    c = network_case(name)
    net = load_gfpgan(c["sd"]).double()
    with torch.no_grad():
        got = net(c["x"])
    assert got.shape == c["a"].shape == (2, 3, c["cfg"]["out_size"], c["cfg"]["out_size"])
    err = float((got - c["a"]).abs().max())
    print(f"GFPGANv1Clean.forward {name}: max |forward - restatement| = {err:.3e} (fp64), output std {float(c['a'].std()):.3f}")
    assert err <= 1e-10


@pytest.mark.parametrize("name", ["32", "64"])
def test_network_references_are_sensitive(name):
    """What tests/test_hip_gfpgan.py can see: with the test weights, zeroed noise weights, a dropped SFT, dropped demodulation, a dropped
    sqrt(2), dropped U-Net skips, nearest instead of bilinear upsampling and swapped scale / shift each move reference A by at least 10 times
    the device bound 2 e16 (levels of 127.5); the output is of order 1, the two samples differ, and e16 is a real number."""
    c = network_case(name)
    bound = 2 * c["e16"]
    assert 0.01 < c["e16"] < 3 and 0.3 < float(c["a"].std()) < 2
    assert LEVELS * float((c["a"][0] - c["a"][1]).abs().max()) >= 10 * bound
    for m in MUTATIONS:
        moved = LEVELS * float((gfpgan_walk(c["sd"], c["x"], c["cfg"], mutate=m) - c["a"]).abs().max())
        print(f"GFPGAN {name} {m}: reference moves by {moved:.1f} levels, device bound {bound:.2f}")
        assert moved >= 10 * bound, (m, moved, bound)


def test_hip_refuses_wrong_inputs_before_any_gpu_work():
    net = GFPGANv1Clean(num_mlp=8, **CFG32)
    for bad in (torch.zeros(1, 32, 32, 8), torch.zeros(1, 32, 32, 8, dtype=torch.float16), torch.zeros(1, 3, 32, 32, dtype=torch.float16), None):
        with pytest.raises(RuntimeError, match="fp16 device tensor"):
            net.hip(bad)
    with pytest.raises(ValueError, match="power of two"):
        GFPGANv1Clean(out_size=48)
    with pytest.raises(ValueError, match="multiples of 8"):
        GFPGANv1Clean(out_size=32, num_style_feat=64, narrow=0.01)


# ---------------------------------------------------------------------------------------------------------------- FaceRestorer, host side
class _NoHip(GFPGANv1Clean):
    def hip(self, crops):
        raise AssertionError("the device path was reached")


def _restorer(detect, **kw):
    net = _NoHip(num_mlp=8, **CFG32)
    net.to = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the network was moved to the device"))
    return FaceRestorer(net, detect, device="cpu", **kw)


def test_template_scales_with_the_crop_size():
    assert FFHQ_TEMPLATE_512.shape == (5, 2) and np.array_equal(ffhq_template(512), FFHQ_TEMPLATE_512)
    assert np.allclose(ffhq_template(32), FFHQ_TEMPLATE_512 / 16, rtol=0, atol=1e-12)
    # landmarks that ARE a similarity image of the template give that similarity back, at the network's size
    th, s, t = 0.3, 1.7, np.array([20.0, 11.0])
    R = s * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    kps = ffhq_template(32) @ R.T + t
    fr = _restorer(lambda rgb: [(0.0, 0.0, 10.0, 10.0, 0.9, kps.tolist())])
    fwd, inv = fr.face_matrices(np.zeros((60, 80, 3), dtype=np.uint8))
    assert fwd.shape == inv.shape == (1, 2, 3) and fwd.dtype == np.float32
    back = kps @ fwd[0, :, :2].astype(np.float64).T + fwd[0, :, 2]
    assert np.abs(back - ffhq_template(32)).max() < 1e-4
    assert np.abs(inv[0].astype(np.float64) - np.concatenate([R, t[:, None]], axis=1)).max() < 1e-5
    assert np.allclose(estimate_similarity(kps, ffhq_template(32))[0], fwd[0], atol=1e-5)


def test_restorer_selects_faces_and_returns_a_faceless_image_unchanged():
    from PIL import Image
    k = lambda dx: (ffhq_template(32) + [dx, 5.0]).tolist()
    faces = [(2.0 + 30 * i, 5.0, 20.0, 20.0, 0.9 - 0.1 * i, k(30.0 * i)) for i in range(3)] + [(0.0, 0.0, 5.0, 5.0, 0.5, None)]
    rgb = np.zeros((60, 100, 3), dtype=np.uint8)                                                # box centres at x = 12, 42, 72
    assert _restorer(lambda im: faces).face_matrices(rgb)[0].shape == (3, 2, 3)                 # the face without landmarks is skipped
    assert _restorer(lambda im: faces, max_faces=2).face_matrices(rgb)[0].shape == (2, 2, 3)
    one = _restorer(lambda im: faces, only_center_face=True).face_matrices(rgb)[0]
    assert one.shape == (1, 2, 3) and abs(one[0, 0, 2] + 30.0) < 1e-3                          # the middle face: shifted back by 30
    seen = []
    fr = _restorer(lambda im: seen.append(im.shape) or [])
    photo = torch.randint(0, 256, (40, 56, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    assert torch.equal(fr.restore_u8(photo), photo) and torch.equal(fr(photo), photo) and seen == [(40, 56, 3)] * 2
    arr = fr(photo.numpy())
    assert isinstance(arr, np.ndarray) and np.array_equal(arr, photo.numpy())
    pil = fr(Image.fromarray(photo.numpy()))
    assert isinstance(pil, Image.Image) and np.array_equal(np.asarray(pil), photo.numpy())
    both = fr([photo, Image.fromarray(photo.numpy())])
    assert torch.is_tensor(both[0]) and isinstance(both[1], Image.Image)
    for bad in (torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(8, 8, 3)):
        with pytest.raises(ValueError, match="uint8 tensor"):
            fr.restore_u8(bad)
    with pytest.raises(ValueError, match="GFPGANv1Clean"):
        FaceRestorer(torch.nn.Conv2d(3, 3, 3), lambda im: [])
    with pytest.raises(ValueError, match="detect_faces"):
        FaceRestorer(GFPGANv1Clean(num_mlp=8, **CFG32), None)
    with pytest.raises(ValueError, match="erode and feather"):
        _restorer(lambda im: [], erode=0.3, feather=0.3)
    with pytest.raises(ValueError, match="max_faces"):
        _restorer(lambda im: [], max_faces=17)


# ---------------------------------------------------------------------------------------------------------------- wrapper
def test_wrapper_loads_and_unloads_a_face_restorer():
    fr = _restorer(lambda im: [])
    w = _wrapper(face_restorer=fr)
    assert w.face_restorer is fr and "face_restorer" not in dict(w.named_modules())
    w.unload_face_restorer()
    assert w.face_restorer is None
    with pytest.raises(ValueError, match="needs a detector"):
        w.load_face_restorer(GFPGANv1Clean(num_mlp=8, **CFG32))
    det = lambda im: []
    got = w.load_face_restorer(make_state_dict(CFG32, seed=3), detect_faces=det, erode=0.1)
    assert got is w.face_restorer and got.detect_faces is det and got.erode == 0.1 and got.size == 32


def test_wrapper_restore_faces_refuses_before_any_gpu_work():
    pe = torch.zeros(1, 77, 64)
    noise = torch.zeros(1, 4, 16, 8)
    w = _wrapper(vae=_vae())
    calls = _spy_apply(w)
    with pytest.raises(ValueError, match="no face restorer is loaded"):
        w(noise, None, prompt_embeds=(pe, pe), out_image_count=1, restore_faces=True)
    w = _wrapper(face_restorer=_restorer(lambda im: []))
    calls += _spy_apply(w)
    with pytest.raises(ValueError, match="needs a vae"):
        w(noise, None, prompt_embeds=(pe, pe), out_image_count=1, restore_faces=True)
    assert calls == []


def test_to_pil_restores_before_it_upscales():
    """_to_pil(latents, upscale, restore_faces): image by image through FaceRestorer.restore_u8 only on request, and the upscaler then sees the
    restored images."""
    w = _wrapper()
    dec = torch.rand(2, 3, 16, 24, generator=torch.Generator().manual_seed(3)) * 2.4 - 1.2
    w.vae = types.SimpleNamespace(decode=lambda z: dec)
    order = []

    def restore_u8(t):
        order.append(("restore", tuple(t.shape)))
        return 255 - t

    def upscale_u8(t):
        order.append(("upscale", tuple(t.shape)))
        return t.repeat_interleave(2, 1).repeat_interleave(2, 2)

    w.__dict__["face_restorer"] = types.SimpleNamespace(restore_u8=restore_u8)
    w.__dict__["upscaler"] = types.SimpleNamespace(upscale_u8=upscale_u8)
    lat = torch.zeros(2, 4, 2, 3)
    want = ((dec / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).numpy()
    plain = w._to_pil(lat)
    assert order == [] and all(np.array_equal(np.asarray(p), q) for p, q in zip(plain, want))
    got = w._to_pil(lat, False, True)
    assert order == [("restore", (16, 24, 3))] * 2 and all(np.array_equal(np.asarray(p), 255 - q) for p, q in zip(got, want))
    del order[:]
    big = w._to_pil(lat, True, True)
    assert order == [("restore", (16, 24, 3))] * 2 + [("upscale", (2, 16, 24, 3))]
    assert np.array_equal(np.asarray(big[1]), (255 - want[1]).repeat(2, 0).repeat(2, 1))


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_header_and_exports_carry_the_kernels():
    with open(os.path.join(ROOT, "include", "adaface_hip.h")) as f:
        header = f.read()
    for name in ("af_modulate_weights", "af_style_epilogue", "af_bilinear_up2", "af_face_paste_affine_u8", "af_face_align_crop_any"):
        assert f"int {name}(const void* " in header and name in _lib.EXPORTS


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """No GPU here: every call below must come back AF_E_BADARG from the argument checks (a launch would fail differently).  Pointers are
    made-up aligned addresses that are never dereferenced."""
    L = _lib.lib()
    P = 1 << 20

    def check(fn, name, good, cases):
        for kw in cases:
            a = dict(good, **kw)
            assert fn(*a.values(), None) == _lib.AF_E_BADARG, (name, kw)
            assert name.encode() + b":" in L.af_last_error(), (name, kw, L.af_last_error())

    check(L.af_modulate_weights, "af_modulate_weights",
          dict(w=P, wsq=2 * P, styles=3 * P, out=4 * P, B=2, cout=24, cin=40, taps=9, npad=128, kpad=384, demod=1, gain=1.0),
          [dict(w=None), dict(styles=None), dict(out=None), dict(wsq=None), dict(cin=36), dict(cin=0), dict(cout=0), dict(B=0), dict(taps=4),
           dict(kpad=320), dict(kpad=400), dict(npad=64), dict(npad=0), dict(cout=129), dict(demod=2), dict(w=P + 4), dict(out=4 * P + 8),
           dict(B=1024, cout=512, cin=512, npad=512, kpad=4608, out=1 << 40, w=1 << 41),               # B * npad * kpad = 2^28 * 9 >= 2^31
           dict(B=70000)])

    check(L.af_style_epilogue, "af_style_epilogue",
          dict(y=P, noise=2 * P, bias=3 * P, scale=4 * P, shift=5 * P, out=6 * P, B=2, HW=35, C=48, nw=0.2),
          [dict(y=None), dict(out=None), dict(C=44), dict(C=0), dict(C=40), dict(B=0), dict(HW=0), dict(noise=None), dict(scale=None),
           dict(shift=None), dict(y=P + 8), dict(scale=4 * P + 2), dict(noise=2 * P + 2), dict(B=16, HW=512 * 512, C=512, y=1 << 40, out=1 << 41)])

    check(L.af_bilinear_up2, "af_bilinear_up2", dict(x=P, addend=None, out=2 * P, B=2, H=3, W=5, C=24),
          [dict(x=None), dict(out=None), dict(C=20), dict(C=0), dict(B=0), dict(H=0), dict(W=-1), dict(x=P + 8), dict(addend=3 * P + 4),
           dict(out=P), dict(out=P + 16 * 24), dict(x=2 * P + 32), dict(B=8, H=512, W=512, C=256, out=1 << 40)])   # 4 B H W C = 2^31

    check(L.af_face_paste_affine_u8, "af_face_paste_affine_u8",
          dict(photo=P, crops=2 * P, mats=3 * P, out=4 * P, H=67, W=91, F=2, S=64, ld=8, erode=3.0, feather=6.0),
          [dict(photo=None), dict(out=None), dict(crops=None), dict(mats=None), dict(F=17), dict(F=-1), dict(S=1), dict(ld=2), dict(H=0), dict(W=0),
           dict(erode=-1.0), dict(feather=-0.5), dict(erode=float("nan")), dict(crops=2 * P + 1), dict(mats=3 * P + 2), dict(out=P + 3),
           dict(H=32768, W=32768, out=1 << 40), dict(F=16, S=4096, ld=8)])                                       # H W 3 and F S S ld >= 2^31

    check(L.af_face_align_crop_any, "af_face_align_crop_any", dict(img=P, inv=2 * P, out=3 * P, H=67, W=91, F=2, size=64),
          [dict(img=None), dict(inv=None), dict(out=None), dict(H=0), dict(W=0), dict(F=0), dict(size=0), dict(size=60), dict(size=1032),
           dict(size=-8), dict(out=3 * P + 8), dict(H=32768, W=32768), dict(F=256, size=1024)])                  # F size^2 8 = 2^31
    # the recogniser's entry keeps its two sizes
    assert L.af_face_align_crop(P, 2 * P, 3 * P, 67, 91, 2, 64, None) == _lib.AF_E_BADARG and b"size must be 112 or 128" in L.af_last_error()
