"""Motion modules on a real MI355X (`pytest -m gpu`), at reduced width (model_channels 64, context 128, 8 x 8 latents, 2 videos of 4 or 8
frames): one TemporalTransformer and the whole U-Net with a v2 module against the plain-torch fp32 CPU walk of tests/motion_util.py
(composed from oracle.unet_oracle's layer functions), the two bitwise properties of the U-Net's motion state, and
AdaFaceWrapper.forward(num_frames=4) under DDIM and DPM-Solver++ against the same walk driven by the samplers' restated updates.

Bounds are the project's existing ones: 2e-3 rel-L2 for one block and 4e-3 for the U-Net (test_hip_unet.BLOCK_TOL / NET_TOL), 3.8e-3 for
a short sampling chain at this width (test_hip_hires)."""
import numpy as np
import pytest
import torch

import dpmpp_restatement as R
from conftest import rel_l2
from motion_util import direct_pe, motion_unet_cfg, synth_motion_sd, temporal_transformer_ref, transformer_shapes, unet_forward_video

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
    """(unet on the device, its CPU state dict, v2 motion state dict, MotionModule on the device)."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    from adaface_dev_amd.ldm.modules.motion_module import MotionModule
    cfg = motion_unet_cfg()
    unet = UNetModel(**cfg)
    rng.load_synth_weights(unet, seed=63)
    sd = {k: v.detach().clone() for k, v in unet.state_dict().items()}
    msd = synth_motion_sd(cfg, with_mid=True, max_len=32, seed=5)
    return unet.to(dev).eval(), sd, msd, MotionModule(msd).to(dev)


def _inputs(nf, seed=21):
    from adaface_dev_amd import rng
    B = 2 * nf
    x = rng.synth_input("motion.x", (B, 4, 8, 8), seed=seed)
    ctx = rng.synth_input("motion.ctx", (2, 77, 128), seed=seed + 1).repeat_interleave(nf, dim=0)       # one prompt per video
    t = torch.tensor([700, 250]).repeat_interleave(nf)
    return x, t, ctx


def _eps(unet, dev, x, t, ctx):
    with torch.no_grad():
        e = unet(x.to(dev), t.to(dev), ctx.to(dev), extra_info={})
    torch.cuda.synchronize()
    return e.cpu()


# ---------------------------------------------------------------------------------------------------------------- one transformer
@pytest.mark.parametrize("C,nf,H,W", [(64, 4, 8, 8), (64, 8, 8, 8), (256, 8, 8, 8), (256, 7, 1, 1), (128, 32, 4, 4)],
                         ids=["c64_f4", "c64_f8_folded_ln", "c256_f8_folded_ln", "c256_f7_one_pixel", "c128_f32"])
def test_temporal_transformer_vs_cpu(dev, C, nf, H, W):
    """2 videos.  512 token rows take the LayerNorm kernel in front of the q|k|v GEMM, 1024 and more the folded form."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.modules.motion_module import TemporalTransformer
    sd = {k: (direct_pe(32, C).float() if k.endswith("pos_encoder.pe") else rng.synth_tensor("tt." + k, s, seed=9).clone())
          for k, s in transformer_shapes(C, 32).items()}
    tt = TemporalTransformer(C, 8, 32)
    tt.load_state_dict(sd, strict=True)
    tt = tt.to(dev)
    x = rng.synth_input("tt.x", (2 * nf, H, W, C), seed=C + nf).to(torch.float16)
    with torch.no_grad():
        y = tt.hip(x.to(dev), nf)
    torch.cuda.synchronize()
    assert y.shape == x.shape and y.dtype == torch.float16
    ref = temporal_transformer_ref(sd, "", x.float().permute(0, 3, 1, 2), nf)
    x_nchw = x.float().permute(0, 3, 1, 2)
    moved = rel_l2(ref.numpy(), x_nchw.numpy())
    err = rel_l2(y.float().cpu().permute(0, 3, 1, 2).numpy(), ref.numpy())
    print(f"TemporalTransformer C={C} F={nf} {H}x{W}: rel-L2 vs the CPU restatement {err:.3e}; the module moves its input by {moved:.3e}")
    assert moved > 0.3                         # the residual it rides on does not hide the module
    assert err < BLOCK_TOL


def test_temporal_transformer_refuses_a_ragged_batch(dev, net):
    _, _, _, mm = net
    tt = mm.at("input", 1)
    x = torch.zeros(10, 8, 8, 64, dtype=torch.float16, device=dev)
    for nf in (4, 0, 33):
        with pytest.raises(ValueError, match="whole videos"):
            tt.hip(x, nf)


# ---------------------------------------------------------------------------------------------------------------- U-Net
@pytest.mark.parametrize("nf", [4, 8])
def test_unet_with_motion_vs_cpu_walk(dev, net, nf):
    unet, sd, msd, mm = net
    x, t, ctx = _inputs(nf)
    e_img = _eps(unet, dev, x, t, ctx)
    unet.set_motion(mm, nf)
    try:
        e_vid = _eps(unet, dev, x, t, ctx)
    finally:
        unet.set_motion(None)
    cfg = motion_unet_cfg()
    with torch.no_grad():
        ref_img = unet_forward_video(sd, None, cfg, x, t, ctx, nf)
        ref_vid = unet_forward_video(sd, msd, cfg, x, t, ctx, nf)
    err_img, err_vid = rel_l2(e_img.numpy(), ref_img.numpy()), rel_l2(e_vid.numpy(), ref_vid.numpy())
    moved = rel_l2(ref_vid.numpy(), ref_img.numpy())
    print(f"U-Net F={nf}: rel-L2 vs the CPU walk {err_vid:.3e} with the motion module, {err_img:.3e} without; the module moves eps by {moved:.3e}")
    assert moved > 0.05                       # the 21 transformers are not a no-op on these weights
    assert err_img < NET_TOL and err_vid < NET_TOL


def test_set_motion_none_restores_the_image_walk_bitwise(dev, net):
    unet, _, _, mm = net
    x, t, ctx = _inputs(4)
    before = _eps(unet, dev, x, t, ctx)
    unet.set_motion(mm, 4)
    try:
        video = _eps(unet, dev, x, t, ctx)
    finally:
        unet.set_motion(None)
    assert not torch.equal(video, before)
    assert torch.equal(_eps(unet, dev, x, t, ctx), before)


def test_zeroed_proj_out_is_the_per_frame_image_output_bitwise(dev, net):
    from adaface_dev_amd.ldm.modules.motion_module import MotionModule
    unet, _, msd, _ = net
    zsd = {k: (torch.zeros_like(v) if ".proj_out." in k else v) for k, v in msd.items()}
    zm = MotionModule(zsd).to(dev)
    x, t, ctx = _inputs(8)
    image = _eps(unet, dev, x, t, ctx)
    unet.set_motion(zm, 8)
    try:
        video = _eps(unet, dev, x, t, ctx)
    finally:
        unet.set_motion(None)
    assert torch.equal(video, image)


def test_unet_refuses_a_batch_of_broken_videos(dev, net):
    unet, _, _, mm = net
    x, t, ctx = _inputs(4)
    unet.set_motion(mm, 3)
    try:
        with pytest.raises(ValueError, match="multiple of num_frames"):
            _eps(unet, dev, x, t, ctx)
    finally:
        unet.set_motion(None)


# ---------------------------------------------------------------------------------------------------------------- wrapper
def _wrapper(dev, scheduler, msd, with_vae=False):
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
    w = AdaFaceWrapper(pipeline_name="text2img", clip_config=cc, ldm=ld, vae=ae, device=dev, num_inference_steps=2,
                       default_scheduler_name=scheduler, motion_module_path=msd)
    return w.to(dev)


@pytest.mark.parametrize("scheduler", ["ddim", "dpm++"])
def test_wrapper_video_vs_cpu_walk(dev, net, scheduler):
    """2 videos of 4 frames, 2 steps, CFG 4, latents out; DDIM with a v2 module, DPM-Solver++ with a v1 module (no mid block, 24 positions).
    The reference drives unet_forward_video with the sampler's restated update (oracle.diffusion_oracle / dpmpp_restatement)."""
    from adaface_dev_amd import rng
    from oracle import diffusion_oracle as D
    _, sd, msd_v2, _ = net
    cfg = motion_unet_cfg()
    msd = msd_v2 if scheduler == "ddim" else synth_motion_sd(cfg, with_mid=False, max_len=24, seed=6)
    nf, videos, g, S = 4, 2, 4.0, 2
    w = _wrapper(dev, scheduler, msd)
    assert w.motion_module.max_len == (32 if scheduler == "ddim" else 24)
    pe = rng.synth_input("motion.pe", (1, 77, 128), seed=85)
    ne = rng.synth_input("motion.ne", (1, 77, 128), seed=86)
    noise = rng.synth_input("motion.noise", (videos * nf, 4, 8, 8), seed=87)
    out = w(noise.to(dev), None, prompt_embeds=(pe.to(dev), ne.to(dev)), guidance_scale=g, out_image_count=videos, num_frames=nf)
    torch.cuda.synchronize()
    assert out.shape == (videos * nf, 4, 8, 8) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    assert w.ldm.model.diffusion_model._motion is None
    B = videos * nf
    c2 = torch.cat([pe.repeat(B, 1, 1), ne.repeat(B, 1, 1)])

    def eps2(x, t):
        with torch.no_grad():
            return unet_forward_video(sd, msd, cfg, torch.cat([x, x]).float(), torch.full((2 * B,), int(t), dtype=torch.long), c2, nf)

    if scheduler == "ddim":
        tabs = D.register_schedule(D.make_beta_schedule_linear())
        ts = D.make_ddim_timesteps(S)
        _, a, ap = D.make_ddim_sampling_parameters(tabs["alphas_cumprod"], ts)
        scales = D.guide_scale_sequence(S, g)
        x = noise
        for i, index in enumerate(range(S - 1, -1, -1)):
            e2 = eps2(x, ts[index])
            x, _ = D.ddim_update(x, D.cfg_combine(e2[:B], e2[B:], scales[i]), float(a[index]), float(ap[index]))
    else:
        ac = R.sd15_alphas_cumprod()
        ts = R.timesteps(S)
        scales = R.guide_scales(S, g)

        def eps_fn(xk, t, i):
            e2 = eps2(xk.float(), t).double()
            return e2[B:] + scales[i] * (e2[:B] - e2[B:])

        x = R.run(ac, ts, R.orders(S), noise, eps_fn)[0][-1].float()
    err = rel_l2(out.cpu().numpy(), x.numpy())
    # the same chain without the module, for the record (profiles/animatediff.txt)
    img = w(noise.to(dev), None, prompt_embeds=(pe.to(dev), ne.to(dev)), guidance_scale=g, out_image_count=B)
    print(f"wrapper video ({scheduler}, {S} steps, F={nf}, CFG {g}) rel-L2 vs the CPU walk: {err:.3e}; "
          f"the module moves the latents by {rel_l2(out.cpu().numpy(), img.cpu().numpy()):.3e}")
    assert err < CHAIN_TOL


def test_wrapper_video_decodes_to_lists_of_frames(dev, net):
    from adaface_dev_amd import rng
    _, _, msd, _ = net
    w = _wrapper(dev, "ddim", msd, with_vae=True)
    pe = rng.synth_input("motion.pe", (1, 77, 128), seed=85).to(dev)
    noise = rng.synth_input("motion.noise", (2 * 3, 4, 8, 8), seed=88).to(dev)
    out = w(noise, None, prompt_embeds=(pe, pe), guidance_scale=1.0, out_image_count=2, num_frames=3)
    assert len(out) == 2 and all(len(v) == 3 for v in out)
    assert all(im.size == (64, 64) for v in out for im in v)
    assert np.asarray(out[0][0]).shape == (64, 64, 3)
