"""ControlNet on a real MI355X (`pytest -m gpu`), on the reduced-width U-Net of motion_util.motion_unet_cfg() (model_channels 64, context 128)
with 8 x 8 latents and 64 x 64 control images: the hint encoder against the fp64 encoder, the U-Net with a ControlNet set against the
plain-torch fp32 CPU walk of tests/controlnet_util.py (whose teeth test_controlnet_host.py asserts), the bitwise properties of the U-Net's
control state, and AdaFaceWrapper.forward(control_image=...) under DDIM, DPM-Solver++ and LCM against the same walk driven by the samplers'
restated updates.

Bounds: BLOCK_TOL / NET_TOL / CHAIN_TOL are test_hip_motion.py's, where they hold this same U-Net with 21 added transformers, a deeper
addition than ControlNet's trunk."""
import numpy as np
import pytest
import torch

import dpmpp_restatement as R
from conftest import rel_l2
from controlnet_util import hint_encoder_ref, synth_control_images, synth_controlnet_sd, unet_forward_control
from motion_util import motion_unet_cfg, synth_motion_sd

pytestmark = pytest.mark.gpu

BLOCK_TOL, NET_TOL, CHAIN_TOL = 2e-3, 4e-3, 3.8e-3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def net(dev):
    """(unet on the device, its CPU state dict, the ControlNet's CPU state dict, the ControlNet on the device)."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.modules.diffusionmodules.controlnet import load_controlnet
    from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    cfg = motion_unet_cfg()
    unet = UNetModel(**cfg)
    rng.load_synth_weights(unet, seed=63)
    sd = {k: v.detach().clone() for k, v in unet.state_dict().items()}
    csd = synth_controlnet_sd(cfg)
    return unet.to(dev).eval(), sd, csd, load_controlnet(csd, cfg).to(dev)


@pytest.fixture(scope="module")
def images():
    return synth_control_images(2, 64, 64)


@pytest.fixture(scope="module")
def hint_ref(net, images):
    """The fp64 hint features of the two control images, computed once and left unchanged."""
    return hint_encoder_ref(net[2], images, torch.float64)


def _inputs(B, seed=41):
    from adaface_dev_amd import rng
    x = rng.synth_input("cn.x", (B, 4, 8, 8), seed=seed)
    ctx = rng.synth_input("cn.ctx", (B, 77, 128), seed=seed + 1)
    t = torch.tensor([700, 250] * (B // 2))
    return x, t, ctx


def _eps(unet, dev, x, t, ctx):
    with torch.no_grad():
        e = unet(x.to(dev), t.to(dev), ctx.to(dev), extra_info={})
    torch.cuda.synchronize()
    return e.cpu()


# ---------------------------------------------------------------------------------------------------------------- hint encoder
def test_hint_features_vs_fp64(dev, net, images, hint_ref):
    _, _, csd, cn = net
    with torch.no_grad():
        h = cn.hint_features(images.to(dev))
    torch.cuda.synchronize()
    assert h.shape == (2, 8, 8, 64) and h.dtype == torch.float16
    err = rel_l2(h.float().cpu().permute(0, 3, 1, 2).numpy(), hint_ref.numpy())
    nosilu = rel_l2(hint_encoder_ref(csd, images, torch.float64, silu=False).numpy(), hint_ref.numpy())
    print(f"hint_features B0=2 64x64: rel-L2 vs the fp64 encoder {err:.3e} (dropping the SiLUs would move it by {nosilu:.3e})")
    assert err < BLOCK_TOL


# ---------------------------------------------------------------------------------------------------------------- U-Net
@pytest.mark.parametrize("scale", [1.0, 0.6])
def test_unet_with_control_vs_cpu_walk(dev, net, images, hint_ref, scale):
    unet, sd, csd, cn = net
    cfg = motion_unet_cfg()
    x, t, ctx = _inputs(2)
    with torch.no_grad():
        hint = cn.hint_features(images.to(dev))
    unet.set_control(cn, hint, scale)
    try:
        e = _eps(unet, dev, x, t, ctx)
    finally:
        unet.set_control(None)
    with torch.no_grad():
        plain = unet_forward_control(sd, None, cfg, x, t, ctx)
        ref = unet_forward_control(sd, csd, cfg, x, t, ctx, scale=scale, hint=hint_ref.float())
    err, moved = rel_l2(e.numpy(), ref.numpy()), rel_l2(ref.numpy(), plain.numpy())
    print(f"U-Net + ControlNet scale {scale}: rel-L2 vs the CPU walk {err:.3e}; the control moves eps by {moved:.3e}")
    assert moved > 0.05
    assert err < NET_TOL


def test_cond_uncond_batch_on_two_hints(dev, net, images, hint_ref):
    """4 rows on 2 hints: row b takes hint b % 2, which is what the samplers' [cond ; uncond] batch needs."""
    unet, sd, csd, cn = net
    x, t, ctx = _inputs(4, seed=45)
    with torch.no_grad():
        hint = cn.hint_features(images.to(dev))
    unet.set_control(cn, hint, 1.0)
    try:
        e = _eps(unet, dev, x, t, ctx)
        state = unet._control
        assert list(state["expanded"]) == [4]
        again = _eps(unet, dev, x, t, ctx)                      # the expanded hint is made once and kept
        assert torch.equal(again, e) and list(state["expanded"]) == [4]
    finally:
        unet.set_control(None)
    with torch.no_grad():
        ref = unet_forward_control(sd, csd, motion_unet_cfg(), x, t, ctx, hint=hint_ref.float().repeat(2, 1, 1, 1))
    err = rel_l2(e.numpy(), ref.numpy())
    print(f"[cond ; uncond] batch, 4 rows on 2 hints: rel-L2 vs the CPU walk {err:.3e}")
    assert err < NET_TOL


def test_set_control_none_restores_the_plain_walk_bitwise(dev, net, images):
    unet, _, _, cn = net
    x, t, ctx = _inputs(2)
    before = _eps(unet, dev, x, t, ctx)
    with torch.no_grad():
        hint = cn.hint_features(images.to(dev))
    unet.set_control(cn, hint, 1.0)
    try:
        controlled = _eps(unet, dev, x, t, ctx)
        unet.set_control_active(False)
        assert torch.equal(_eps(unet, dev, x, t, ctx), before)   # switched off between two steps (a guidance window): the plain walk
        unet.set_control_active(True)
        assert torch.equal(_eps(unet, dev, x, t, ctx), controlled)
    finally:
        unet.set_control(None)
    assert not torch.equal(controlled, before)
    assert torch.equal(_eps(unet, dev, x, t, ctx), before)


def test_joins_never_write_a_tensor_whose_partials_are_trusted(dev, net, images):
    """Every joined skip is a fresh tensor (not the U-Net's own) and, where it carries GroupNorm partials, they are its own."""
    from adaface_dev_amd import ops
    from adaface_dev_amd.ldm.modules.diffusionmodules.util import to_nhwc_f16
    unet, _, _, cn = net
    x, t, ctx = _inputs(2)
    with torch.no_grad():
        hint = cn.hint_features(images.to(dev))
        xh = to_nhwc_f16(x.to(dev), 8)
        c16 = ctx.to(dev).half()
        skips = [torch.randn(2, s, s, c, device=dev).half() for c, s in zip([64] * 4 + [128] * 3 + [256] * 5, [8] * 3 + [4] * 3 + [2] * 3 + [1] * 3)]
        keep = [s.clone() for s in skips]
        joined, mid = cn.hip_walk(xh, t.to(dev), c16, hint, skips, 1.0)
    torch.cuda.synchronize()
    assert len(joined) == 12 and mid.shape == (2, 1, 1, 256)
    for j, s, k in zip(joined, skips, keep):
        assert j.data_ptr() != s.data_ptr() and torch.equal(s, k)
        gn = getattr(j, "_gn_partials", None)
        assert gn is None or ops.partials_of(j) is gn


@pytest.fixture(scope="module")
def motion(dev):
    from adaface_dev_amd.ldm.modules.motion_module import MotionModule
    msd = synth_motion_sd(motion_unet_cfg(), with_mid=True, max_len=32, seed=5)
    return msd, MotionModule(msd).to(dev)


def test_unet_with_control_and_motion_vs_cpu_walk(dev, net, motion):
    """2 videos of 4 frames, one control image per frame: the U-Net runs the temporal transformers, the ControlNet runs per frame."""
    unet, sd, csd, cn = net
    msd, mm = motion
    nf = 4
    x, t, ctx = _inputs(2 * nf, seed=51)
    t = torch.tensor([700, 250]).repeat_interleave(nf)
    imgs = synth_control_images(2 * nf, 64, 64, seed=9)
    with torch.no_grad():
        hint = cn.hint_features(imgs.to(dev))
    unet.set_motion(mm, nf)
    unet.set_control(cn, hint, 1.0)
    try:
        e = _eps(unet, dev, x, t, ctx)
    finally:
        unet.set_control(None)
        unet.set_motion(None)
    cfg = motion_unet_cfg()
    with torch.no_grad():
        ref = unet_forward_control(sd, csd, cfg, x, t, ctx, imgs, msd=msd, nf=nf)
        no_control = unet_forward_control(sd, None, cfg, x, t, ctx, msd=msd, nf=nf)
        no_motion = unet_forward_control(sd, csd, cfg, x, t, ctx, imgs)
    err = rel_l2(e.numpy(), ref.numpy())
    print(f"U-Net + ControlNet + motion module F={nf}: rel-L2 vs the CPU walk {err:.3e}; without the control the walk differs by "
          f"{rel_l2(no_control.numpy(), ref.numpy()):.3e}, without the motion module by {rel_l2(no_motion.numpy(), ref.numpy()):.3e}")
    assert rel_l2(no_control.numpy(), ref.numpy()) > 0.05 and rel_l2(no_motion.numpy(), ref.numpy()) > 0.05
    assert err < NET_TOL


def test_ragged_batch_wrong_size_and_training_are_refused(dev, net, images):
    unet, _, _, cn = net
    with torch.no_grad():
        hint = cn.hint_features(images.to(dev))
    unet.set_control(cn, hint, 1.0)
    try:
        x, t, ctx = _inputs(2)
        x3, t3, c3 = torch.cat([x, x[:1]]), torch.cat([t, t[:1]]), torch.cat([ctx, ctx[:1]])
        with pytest.raises(ValueError, match="the batch \\(3\\) is not a multiple of the hint batch \\(2\\)"):
            _eps(unet, dev, x3, t3, c3)
        from adaface_dev_amd import rng
        with pytest.raises(ValueError, match="the hints are for 8 x 8 latents"):
            _eps(unet, dev, rng.synth_input("cn.x16", (2, 4, 16, 16), seed=1), t, ctx)
        xg = x.to(dev).requires_grad_(True)
        with pytest.raises(NotImplementedError, match="training is not built with a ControlNet"):
            unet(xg, t.to(dev), ctx.to(dev), extra_info={})
        with pytest.raises(NotImplementedError, match="captured / score-rewrite path is not built with a ControlNet"):
            with torch.no_grad():
                unet(x.to(dev), t.to(dev), ctx.to(dev), extra_info={"normalize_cross_attn": True})
    finally:
        unet.set_control(None)


# ---------------------------------------------------------------------------------------------------------------- wrapper
def _lcm_lora(unet):
    from test_lcm_host import restated_targets, synth_lora
    return synth_lora(unet, restated_targets(), 8, seed=31, alpha=4, scale=0.5)


def _wrapper(dev, scheduler, controlnet, pipeline_name="text2img", with_vae=False, steps=4):
    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper
    from adaface_dev_amd.adaface.arc2face_models import clip_text_config
    from adaface_dev_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    from test_vae_oracle import VAE_SMALL
    cc = clip_text_config(hidden_size=128, num_attention_heads=2, num_hidden_layers=3, intermediate_size=512)
    ld = LatentDiffusion(motion_unet_cfg())
    rng.load_synth_weights(ld.model.diffusion_model, seed=63)
    ae = None
    if with_vae:
        ae = ld.instantiate_first_stage(dict(VAE_SMALL, double_z=True))
        with torch.no_grad():
            for n, p in ae.named_parameters():
                p.copy_(rng.synth_tensor(n, p.shape, seed=92))
    kw = dict(use_lcm=True, lcm_lora_path=_lcm_lora(ld.model.diffusion_model)) if scheduler == "lcm" else dict(default_scheduler_name=scheduler)
    w = AdaFaceWrapper(pipeline_name=pipeline_name, clip_config=cc, ldm=ld, vae=ae, device=dev, num_inference_steps=steps, controlnet=controlnet, **kw)
    return w.to(dev)


def _cpu_chain(scheduler, sd, csd, hint, noise, pe, ne, g, S, active):
    """The sampler's restated update driving the CPU walk; control on in the steps of ``active``.  LCM re-noises from seed 3."""
    from oracle import diffusion_oracle as D
    cfg = motion_unet_cfg()
    B = noise.shape[0]
    c2 = torch.cat([pe.repeat(B, 1, 1), ne.repeat(B, 1, 1)])

    def eps2(x, t, i):
        with torch.no_grad():
            return unet_forward_control(sd, csd if i in active else None, cfg, torch.cat([x, x]).float(), torch.full((2 * B,), int(t), dtype=torch.long),
                                        c2, hint=hint)

    if scheduler == "ddim":
        tabs = D.register_schedule(D.make_beta_schedule_linear())
        ts = D.make_ddim_timesteps(S)
        _, a, ap = D.make_ddim_sampling_parameters(tabs["alphas_cumprod"], ts)
        scales = D.guide_scale_sequence(S, g)
        x = noise
        for i, index in enumerate(range(S - 1, -1, -1)):
            e2 = eps2(x, ts[index], i)
            x, _ = D.ddim_update(x, D.cfg_combine(e2[:B], e2[B:], scales[i]), float(a[index]), float(ap[index]))
        return x
    if scheduler == "dpm++":
        ac = R.sd15_alphas_cumprod()
        ts = R.timesteps(S)
        scales = R.guide_scales(S, g)

        def eps_fn(xk, t, i):
            e2 = eps2(xk.float(), t, i).double()
            return e2[B:] + scales[i] * (e2[:B] - e2[B:])

        return R.run(ac, ts, R.orders(S), noise, eps_fn)[0][-1].float()
    from adaface_dev_amd.ldm.models.diffusion.lcm import lcm_step_coefficients, lcm_timesteps
    ac = R.sd15_alphas_cumprod()
    ts = lcm_timesteps(S).tolist()
    gen = torch.Generator().manual_seed(3)
    x = noise.double()
    for i, (t, (sa, sb, c_out, c_skip, sa_n, sb_n)) in enumerate(zip(ts, lcm_step_coefficients(np.asarray(ac, dtype=np.float64), ts))):
        e2 = eps2(x.float(), t, i).double()
        e = e2[B:] + g * (e2[:B] - e2[B:])
        d = c_out * (x - sb * e) / sa + c_skip * x
        x = sa_n * d + sb_n * torch.randn(x.shape, generator=gen).double() if i < S - 1 else d
    return x.float()


@pytest.mark.parametrize("scheduler", ["ddim", "dpm++", "lcm"])
def test_wrapper_text2img_vs_cpu_chain(dev, net, images, hint_ref, scheduler):
    """2 rows, 4 steps, CFG, latents out (vae=None), one control image per row: the whole window, then the window (0, 0.5) = steps 0 and 1."""
    from adaface_dev_amd import rng
    _, sd, csd, _ = net
    g, S, B = (1.5 if scheduler == "lcm" else 4.0), 4, 2
    w = _wrapper(dev, scheduler, csd)
    if scheduler == "lcm":
        from test_lcm_host import fused_state_dict, restated_targets
        sd = fused_state_dict(sd, _lcm_lora(w.ldm.model.diffusion_model), restated_targets())
    pe = rng.synth_input("cn.pe", (1, 77, 128), seed=85)
    ne = rng.synth_input("cn.ne", (1, 77, 128), seed=86)
    noise = rng.synth_input("cn.noise", (B, 4, 8, 8), seed=87)
    run = lambda **kw: w(noise.to(dev), None, prompt_embeds=(pe.to(dev), ne.to(dev)), guidance_scale=g, out_image_count=B,
                         generator=torch.Generator().manual_seed(3), **kw).cpu()
    plain = run()
    hint = hint_ref.float()
    for (start, end), active in (((0.0, 1.0), {0, 1, 2, 3}), ((0.0, 0.5), {0, 1})):
        out = run(control_image=images, control_guidance_start=start, control_guidance_end=end)
        torch.cuda.synchronize()
        assert out.shape == (B, 4, 8, 8) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
        assert w.ldm.model.diffusion_model._control is None
        ref = _cpu_chain(scheduler, sd, csd, hint, noise, pe, ne, g, S, active)
        err = rel_l2(out.numpy(), ref.numpy())
        print(f"wrapper text2img ({scheduler}, {S} steps, CFG {g}, window {start}-{end}) rel-L2 vs the CPU chain: {err:.3e}; "
              f"the control moves the latents by {rel_l2(out.numpy(), plain.numpy()):.3e}")
        assert rel_l2(out.numpy(), plain.numpy()) > 0.05
        assert err < CHAIN_TOL


@pytest.mark.parametrize("pipeline", ["img2img", "inpaint"])
def test_wrapper_img2img_and_inpaint_take_a_control_image(dev, net, images, pipeline):
    from PIL import Image
    from adaface_dev_amd import rng
    _, _, csd, _ = net
    w = _wrapper(dev, "ddim", csd, pipeline_name=pipeline, with_vae=True)
    pe = rng.synth_input("cn.pe", (1, 77, 128), seed=85).to(dev)
    photo = Image.fromarray(synth_control_images(1, 64, 64, seed=21)[0].numpy())
    extra = {}
    if pipeline == "inpaint":
        m = np.zeros((64, 64), dtype=np.uint8)
        m[16:48, 8:56] = 255
        extra["mask_image"] = Image.fromarray(m)
    run = lambda **kw: w(photo, None, prompt_embeds=(pe, pe), guidance_scale=3.0, out_image_count=2, ref_img_strength=0.75,
                         generator=torch.Generator(device=dev).manual_seed(4), **extra, **kw)
    plain = run()
    out = run(control_image=Image.fromarray(images[0].numpy()), control_scale=0.8)
    assert w.ldm.model.diffusion_model._control is None
    assert len(out) == 2 and all(im.size == (64, 64) for im in out)
    a, b = np.stack([np.asarray(im) for im in out]), np.stack([np.asarray(im) for im in plain])
    assert a.shape == b.shape and not np.array_equal(a, b)
    again = run()
    assert all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(again, plain))


def test_forward_without_control_image_is_bitwise_the_wrapper_without_a_controlnet(dev, net):
    from adaface_dev_amd import rng
    _, _, csd, _ = net
    pe = rng.synth_input("cn.pe", (1, 77, 128), seed=85).to(dev)
    ne = rng.synth_input("cn.ne", (1, 77, 128), seed=86).to(dev)
    noise = rng.synth_input("cn.noise", (2, 4, 8, 8), seed=87).to(dev)
    outs = [_wrapper(dev, "ddim", c, steps=2)(noise, None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=2) for c in (None, csd)]
    assert torch.equal(outs[0], outs[1])
