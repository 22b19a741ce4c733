"""ControlNet without a GPU: the loader, the teeth of the CPU reference walk the GPU tests compare against (tests/controlnet_util.py), the
guidance-window rule, every refusal of AdaFaceWrapper.forward(control_image=...) on a CPU-only wrapper, U-Net.set_control's refusals and
af_hint_conv3x3's argument checks."""
import ctypes
import os

import numpy as np
import pytest
import torch

from adaface_dev_amd import _lib, rng
from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper, control_images_u8
from adaface_dev_amd.adaface.arc2face_models import clip_text_config
from adaface_dev_amd.ldm.modules.diffusionmodules.controlnet import ControlNet, guidance_window_active, load_controlnet
from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel, unet_param_shapes
from conftest import rel_l2
from controlnet_util import FAULTS, ZERO_GAIN, controlnet_shapes, synth_control_images, synth_controlnet_sd, unet_forward_control
from motion_util import motion_unet_cfg, synth_motion_sd
from oracle import unet_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET_TOL = 4e-3             # test_hip_controlnet.NET_TOL: a fault of the walk must move eps by more than ten times what the GPU test allows


@pytest.fixture(scope="module")
def cfg():
    return motion_unet_cfg()


@pytest.fixture(scope="module")
def csd(cfg):
    return synth_controlnet_sd(cfg)


# ---------------------------------------------------------------------------------------------------------------- loader
def test_loader_bare_prefixed_and_v10_files(cfg, csd, tmp_path):
    net = load_controlnet(csd, cfg)
    assert isinstance(net, ControlNet) and not net.training
    own = net.state_dict()
    assert set(own) == set(csd) == set(controlnet_shapes(cfg))
    assert all(torch.equal(own[k], csd[k]) for k in csd)
    pre = load_controlnet({"control_model." + k: v for k, v in csd.items()}, cfg)
    assert all(torch.equal(pre.state_dict()[k], csd[k]) for k in csd)
    # a v1.0-style file also holds the whole SD-1.5 model: once a key carries the prefix, only prefixed keys are read
    v10 = {"control_model." + k: v for k, v in csd.items()}
    v10.update({"model.diffusion_model." + n: torch.zeros(1) for n, _ in unet_param_shapes(cfg)[:5]})
    v10["first_stage_model.decoder.conv_in.weight"] = torch.zeros(1)
    both = load_controlnet(v10, cfg)
    assert all(torch.equal(both.state_dict()[k], csd[k]) for k in csd)
    # files: a torch file with a "state_dict" wrapper
    path = tmp_path / "control_synth.pth"
    torch.save({"state_dict": v10}, path)
    from_file = load_controlnet(str(path), cfg).state_dict()
    assert all(torch.equal(from_file[k], csd[k]) for k in csd)
    # the published names are all there
    for k in ("time_embed.0.weight", "time_embed.2.bias", "input_blocks.0.0.weight", "input_blocks.11.0.out_layers.3.weight",
              "middle_block.1.proj_in.weight", "input_hint_block.0.weight", "input_hint_block.14.bias", "zero_convs.0.0.weight",
              "zero_convs.11.0.bias", "middle_block_out.0.weight"):
        assert k in own, k
    assert tuple(own["input_hint_block.4.weight"].shape) == (32, 16, 3, 3) and tuple(own["input_hint_block.12.weight"].shape) == (256, 96, 3, 3)


def test_loader_is_strict_and_names_the_key(cfg, csd):
    missing = {k: v for k, v in csd.items() if k != "zero_convs.7.0.bias"}
    with pytest.raises(ValueError, match=r"missing: \['zero_convs\.7\.0\.bias'\]"):
        load_controlnet(missing, cfg)
    with pytest.raises(ValueError, match=r"unexpected: \['input_hint_block\.16\.weight'\]"):
        load_controlnet(dict(csd, **{"input_hint_block.16.weight": torch.zeros(4)}), cfg)
    bad = dict(csd, **{"input_hint_block.2.weight": torch.zeros(16, 16, 1, 1)})
    with pytest.raises(ValueError, match=r"wrong shape: \['input_hint_block\.2\.weight \(16, 16, 1, 1\) \(expected \(16, 16, 3, 3\)\)"):
        load_controlnet(bad, cfg)
    # the prefixed form reports bare names too; a bare key next to prefixed ones is simply not read, so the prefixed set must be whole
    pre = {"control_model." + k: v for k, v in missing.items()}
    pre["zero_convs.7.0.bias"] = csd["zero_convs.7.0.bias"]
    with pytest.raises(ValueError, match="missing.*zero_convs.7.0.bias"):
        load_controlnet(pre, cfg)
    # another U-Net's ControlNet
    with pytest.raises(ValueError, match="wrong shape"):
        load_controlnet(csd, dict(cfg, model_channels=128))


def test_loader_refuses_the_diffusers_layout_by_name(cfg):
    sd = {"controlnet_cond_embedding.conv_in.weight": torch.zeros(16, 3, 3, 3), "controlnet_down_blocks.0.weight": torch.zeros(4, 4, 1, 1),
          "down_blocks.0.resnets.0.conv1.weight": torch.zeros(4, 4, 3, 3)}
    with pytest.raises(ValueError, match="diffusers ControlNetModel layout.*not read"):
        load_controlnet(sd, cfg)


# ---------------------------------------------------------------------------------------------------------------- reference teeth
def _inputs():
    x = rng.synth_input("cn.x", (2, 4, 8, 8), seed=41)
    ctx = rng.synth_input("cn.ctx", (2, 77, 128), seed=42)
    return x, torch.tensor([700, 250]), ctx, synth_control_images(2, 64, 64)


def test_reference_teeth(cfg, csd):
    """The CPU walk the GPU tests trust: without control (scale 0) it IS unet_oracle.unet_forward; with the synthetic zero convolutions at
    ZERO_GAIN the control moves eps by far more than the GPU tolerance, and so does each single fault of the walk."""
    unet = UNetModel(**cfg)
    rng.load_synth_weights(unet, seed=63)
    sd = {k: v.detach().clone() for k, v in unet.state_dict().items()}
    x, t, ctx, imgs = _inputs()
    with torch.no_grad():
        plain = O.unet_forward(sd, cfg, x, t, ctx, {})
        assert torch.equal(unet_forward_control(sd, csd, cfg, x, t, ctx, imgs, scale=0.0), plain)
        assert torch.equal(unet_forward_control(sd, None, cfg, x, t, ctx), plain)
        good = unet_forward_control(sd, csd, cfg, x, t, ctx, imgs, scale=1.0)
        moved = rel_l2(good.numpy(), plain.numpy())
        print(f"zero_gain {ZERO_GAIN}: the control moves eps by {moved:.3e}")
        assert moved > 0.05
        assert rel_l2(unet_forward_control(sd, csd, cfg, x, t, ctx, imgs, scale=0.6).numpy(), good.numpy()) > 10 * NET_TOL
        for fault in FAULTS:
            d = rel_l2(unet_forward_control(sd, csd, cfg, x, t, ctx, imgs, scale=1.0, fault=fault).numpy(), good.numpy())
            print(f"fault {fault}: eps moves by {d:.3e}")
            assert d > 10 * NET_TOL, (fault, d)
        # hints swapped between the two rows are seen too (row b takes image b % B0)
        d = rel_l2(unet_forward_control(sd, csd, cfg, x, t, ctx, imgs.flip(0)).numpy(), good.numpy())
        print(f"hints of the two rows swapped: eps moves by {d:.3e}")
        assert d > 10 * NET_TOL


# ---------------------------------------------------------------------------------------------------------------- guidance window
@pytest.mark.parametrize("start,end,steps", [(0.0, 1.0, [0, 1, 2, 3]), (0.0, 0.5, [0, 1]), (0.5, 1.0, [2, 3]), (0.25, 0.75, [1, 2])])
def test_guidance_window_rule(start, end, steps):
    assert [i for i in range(4) if guidance_window_active(i, 4, start, end)] == steps


def test_wrapper_switches_control_by_the_window(csd64):
    """forward drives a recording sampler: the ControlNet is on the U-Net during the call only, and the callback forward hands to the
    sampler switches it by the rule (state seen BEFORE each step)."""
    w = _wrapper(controlnet=csd64, num_inference_steps=4)
    unet = w.ldm.model.diffusion_model
    w.controlnet.hint_features = lambda images: torch.zeros(images.shape[0], 8, 8, 64, dtype=torch.float16)
    seen = []

    class Rec:
        def timesteps(self, S):
            return list(range(S))

        def sample(self, S, batch_size, shape, callback=None, **kw):
            for i in range(S):
                seen.append(unet._control is not None and unet._control["active"])
                callback(i)
            return kw["x_T"], {}

    w._sampler = lambda: Rec()
    pe = torch.zeros(1, 77, 64)
    img = synth_control_images(1, 64, 64)[0]
    for (start, end), want in (((0.0, 1.0), [True] * 4), ((0.0, 0.5), [True, True, False, False]), ((0.25, 0.75), [False, True, True, False])):
        seen.clear()
        w(torch.zeros(2, 4, 8, 8), None, prompt_embeds=(pe, pe), out_image_count=2, control_image=img, control_guidance_start=start,
          control_guidance_end=end)
        assert seen == want and unet._control is None


# ---------------------------------------------------------------------------------------------------------------- refusals
def _wrapper(pipeline_name="text2img", **kw):
    cc = clip_text_config(hidden_size=64, num_attention_heads=1, num_hidden_layers=1, intermediate_size=128)
    return AdaFaceWrapper(pipeline_name=pipeline_name, clip_config=cc, unet_config=dict(motion_unet_cfg(), context_dim=64), device="cpu", **kw)


def _spy_apply(w):
    calls = []

    def spy(*a, **k):
        calls.append(a)
        raise AssertionError("the U-Net was reached")

    w.ldm.apply_model = spy
    return calls


@pytest.fixture(scope="module")
def csd64():
    return synth_controlnet_sd(dict(motion_unet_cfg(), context_dim=64))


def test_wrapper_refusals_need_no_gpu(csd64):
    from PIL import Image
    from test_inpaint_host import _vae
    pe = torch.zeros(1, 77, 64)
    noise = torch.zeros(2, 4, 8, 8)
    img = Image.fromarray(synth_control_images(1, 64, 64)[0].numpy())
    w = _wrapper()
    calls = _spy_apply(w)
    run = lambda wr=w, n=noise, **kw: wr(n, None, prompt_embeds=(pe, pe), out_image_count=2, **kw)
    with pytest.raises(ValueError, match="no ControlNet is loaded"):
        run(control_image=img)
    assert w.load_controlnet(csd64) is w.controlnet
    assert not any("zero_convs" in k or "input_hint_block" in k for k in w.state_dict())
    hint = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the hint encoder was reached"))
    w.controlnet.hint_features = hint
    for size in ((63, 64), (128, 128), (32, 32), (64, 72)):
        with pytest.raises(ValueError, match="exactly 8 x the latent size"):
            run(control_image=img.resize(size))
    with pytest.raises(ValueError, match="1 image \\(shared\\) or one per sampled row \\(2\\) expected, got 3"):
        run(control_image=[img] * 3)
    w.load_motion_module(synth_motion_sd(dict(motion_unet_cfg(), context_dim=64), with_mid=False, max_len=24))
    with pytest.raises(ValueError, match="one per sampled row \\(6\\)"):                      # with num_frames the rows are V * F
        run(n=torch.zeros(6, 4, 8, 8), num_frames=3, control_image=[img] * 2)
    with pytest.raises(ValueError, match="control_image must be a PIL image"):
        run(control_image=torch.zeros(64, 64, 3))
    with pytest.raises(ValueError, match="same size"):
        run(control_image=[img, img.resize((32, 32))])
    for s in (float("nan"), float("inf"), -float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="control_scale must be a finite number"):
            run(control_image=img, control_scale=s)
    for start, end in ((-0.1, 1.0), (0.0, 1.1), (0.5, 0.5), (0.7, 0.3), (None, 1.0), (0.0, "1")):
        with pytest.raises(ValueError, match="0 <= control_guidance_start < control_guidance_end <= 1"):
            run(control_image=img, control_guidance_start=start, control_guidance_end=end)
    with pytest.raises(ValueError, match="control_image together with hires_size"):
        run(control_image=img, hires_size=(128, 128))
    assert calls == [] and w.ldm.model.diffusion_model._control is None
    # the inpaint pipeline: no hints under a working size the face finder picks
    wi = _wrapper("inpaint", vae=_vae(), controlnet=csd64, face_detector=lambda rgb: (_ for _ in ()).throw(AssertionError("detector reached")))
    calls_i = _spy_apply(wi)
    with pytest.raises(ValueError, match="control_image together with mask_image='face'"):
        wi(img, None, prompt_embeds=(pe, pe), out_image_count=2, mask_image="face", control_image=img)
    with pytest.raises(ValueError, match="exactly 8 x the latent size"):
        wi(img, None, prompt_embeds=(pe, pe), out_image_count=2, mask_image=img.convert("L"), control_image=img.resize((128, 128)))
    assert calls_i == []
    w.unload_controlnet()
    with pytest.raises(ValueError, match="no ControlNet is loaded"):
        run(control_image=img)
    # a ControlNet of another width is refused at load time
    with pytest.raises(ValueError, match="wrong shape"):
        w.load_controlnet(synth_controlnet_sd(dict(motion_unet_cfg(), model_channels=128, context_dim=64)))
    assert w.controlnet is None


def test_control_images_forms():
    from PIL import Image
    t = synth_control_images(2, 16, 24)
    assert torch.equal(control_images_u8(t, 2), t)
    assert torch.equal(control_images_u8(t[0], 5), t[:1])
    assert torch.equal(control_images_u8([t[0], t[1]], 2), t)
    assert torch.equal(control_images_u8(Image.fromarray(t[1].numpy()), 3), t[1:])
    assert torch.equal(control_images_u8([Image.fromarray(t[0].numpy()), t[1]], 2), t)
    grey = Image.fromarray(t[0, :, :, 0].numpy())                      # an "L" scribble / edge map becomes RGB
    assert torch.equal(control_images_u8(grey, 1), t[:1, :, :, :1].expand(1, 16, 24, 3))


def test_without_control_image_forward_is_the_old_call(csd64):
    """One sampler.sample call with the arguments forward has always passed (no callback); the U-Net's control state is never set."""
    w = _wrapper(num_inference_steps=10, controlnet=csd64)
    log = []

    class Rec:
        def sample(self, S, batch_size, shape, **kw):
            log.append((S, batch_size, tuple(shape), sorted(kw), w.ldm.model.diffusion_model._control))
            return kw["x_T"] + 1.0, {}

    w._sampler = lambda: Rec()
    pe = torch.zeros(1, 77, 64)
    noise = torch.zeros(3, 4, 8, 8)
    out = w(noise, None, prompt_embeds=(pe, pe), out_image_count=3)
    keys = ["conditioning", "generator", "guidance_scale", "unconditional_conditioning", "verbose", "x_T"]
    assert log == [(10, 3, (4, 8, 8), keys, None)] and torch.equal(out, noise + 1.0)


def test_set_control_refusals(cfg, csd):
    unet = UNetModel(**cfg)
    net = load_controlnet(csd, cfg)
    hint = torch.zeros(2, 8, 8, 64, dtype=torch.float16)
    unet.set_control(net, hint, 0.5)
    assert unet._control["net"] is net and unet._control["scale"] == 0.5 and not any("zero_convs" in k for k in unet.state_dict())
    for what, call in (("hip_train", lambda: unet.hip_train(None, None, None)), ("hip_trunk", lambda: unet.hip_trunk(None, None, None, None, 3)),
                       ("hip_tail", lambda: unet.hip_tail((None, []), None, None, ())),
                       ("hip_train_trunk", lambda: unet.hip_train_trunk(None, None, None, None, 3))):
        with pytest.raises(NotImplementedError, match="not built with a ControlNet"):
            call()
    unet.set_control(None)
    assert unet._control is None
    with pytest.raises(ValueError, match="hint_features must be fp16"):
        unet.set_control(net, hint.float())
    with pytest.raises(ValueError, match="hint_features must be fp16"):
        unet.set_control(net, torch.zeros(2, 8, 8, 32, dtype=torch.float16))
    with pytest.raises(ValueError, match="scale must be finite"):
        unet.set_control(net, hint, float("nan"))
    wide = dict(cfg, model_channels=128)
    with pytest.raises(ValueError, match="model_channels is 128, the U-Net's 64"):
        unet.set_control(ControlNet(**wide), torch.zeros(2, 8, 8, 128, dtype=torch.float16))
    with pytest.raises(ValueError, match="channel_mult"):
        unet.set_control(ControlNet(**dict(cfg, channel_mult=[1, 2, 2, 4])), hint)
    with pytest.raises(ValueError, match="attention_resolutions"):
        unet.set_control(ControlNet(**dict(cfg, attention_resolutions=[4, 2])), hint)
    with pytest.raises(ValueError, match="context_dim is 64, the U-Net's 128"):
        unet.set_control(ControlNet(**dict(cfg, context_dim=64)), hint)
    assert unet._control is None
    with pytest.raises(ValueError, match="control images must be uint8"):
        net.hint_features(torch.zeros(1, 60, 64, 3, dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_entry_point_is_declared_exported_and_checks_its_arguments():
    with open(os.path.join(ROOT, "include", "adaface_hip.h")) as f:
        header = " ".join(f.read().split())
    assert ("int af_hint_conv3x3(const void* x, int in_mode, int cin, const void* wt, const void* bias, void* out, int cout, int stride, "
            "int act, int B, int H, int W, void* stream);") in header
    assert "af_hint_conv3x3" in _lib.EXPORTS
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096 + 16)                       # host memory: every call below must be refused before any launch
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    call = lambda x=p, mode=0, cin=16, wt=p, bias=p, out=p, cout=16, s=1, act=1, B=1, H=4, W=4: \
        L.af_hint_conv3x3(x, mode, cin, wt, bias, out, cout, s, act, B, H, W, None)
    for kw in (dict(x=None), dict(wt=None), dict(out=None), dict(cin=0), dict(cin=8), dict(cin=24), dict(cin=272), dict(cin=3), dict(mode=1, cin=16),
               dict(mode=1, cin=4), dict(mode=2), dict(mode=-1), dict(cout=0), dict(cout=8), dict(cout=40), dict(cout=272), dict(s=0), dict(s=3),
               dict(s=-1), dict(act=2), dict(B=0), dict(H=0), dict(W=-1), dict(x=p + 2), dict(wt=p + 8), dict(out=p + 4), dict(bias=p + 2),
               dict(B=2, H=1 << 13, W=1 << 13, cin=16),                      # input of 2^31 elements
               dict(B=1, H=1 << 12, W=1 << 12, cin=16, cout=128),            # output of 2^31 elements
               dict(mode=1, cin=3, B=1 << 10, H=1 << 10, W=1 << 10),         # uint8 image of 3 * 2^30 bytes
               dict(B=1, H=1 << 21, W=1, cin=16),                            # more than 65535 patch rows
               dict(B=1 << 15, H=1, W=1, cin=16, cout=256)):                 # images x channel slabs above 65535
        assert call(**kw) == _lib.AF_E_BADARG, kw
        assert b"af_hint_conv3x3" in L.af_last_error(), kw
