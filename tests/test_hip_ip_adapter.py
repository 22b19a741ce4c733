"""IP-Adapter on a real MI355X (`pytest -m gpu`), on the reduced-width U-Net of motion_util.motion_unet_cfg() (model_channels 64, context 128,
head dims 8 to 32) with 8 x 8 latents: the image projection of both kinds against fp64, the U-Net with an adapter set against the plain-torch
fp32 CPU walk of tests/ip_adapter_util.py (whose teeth test_ip_adapter_host.py asserts), the bitwise properties of the U-Net's adapter state,
the combinations with a ControlNet and a motion module, AdaFaceWrapper.forward(ip_adapter_image= / ip_adapter_face_id=) under DDIM,
DPM-Solver++ and LCM against the same walk driven by the samplers' restated updates, one full-width C = 320 block that otherwise runs as one
launch, and the ViT-H/14 image encoder at reduced depth.

Bounds: BLOCK_TOL / NET_TOL / CHAIN_TOL are test_hip_motion.py's, where they hold this same U-Net with 21 added transformers, a deeper
addition than 16 small attention adds.  FEAT_BOUND is test_hip_eval.py's bound for the vision towers."""
import numpy as np
import pytest
import torch

import dpmpp_restatement as R
import vit_restatement as VR
from conftest import rel_l2
from controlnet_util import synth_control_images, synth_controlnet_sd
from ip_adapter_util import fused_unet_sd, image_proj_ref, ip_inputs, ip_spatial_transformer, synth_ip_sd, unet_forward_ip
from motion_util import motion_unet_cfg, synth_motion_sd

pytestmark = pytest.mark.gpu

BLOCK_TOL, NET_TOL, CHAIN_TOL = 2e-3, 4e-3, 3.8e-3
FEAT_BOUND = 5e-3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def net(dev):
    """(unet on the device, its CPU state dict)."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    unet = UNetModel(**motion_unet_cfg())
    rng.load_synth_weights(unet, seed=63)
    sd = {k: v.detach().clone() for k, v in unet.state_dict().items()}
    return unet.to(dev).eval(), sd


@pytest.fixture(scope="module")
def adapters(dev):
    """{(kind, T): (the synthetic file's state dict, the IPAdapter on the device)}, built once."""
    from adaface_dev_amd.adaface.ip_adapter import load_ip_adapter
    cfg, out = motion_unet_cfg(), {}
    for kind, T in (("clip", 4), ("clip", 16), ("faceid", 4)):
        ipsd = synth_ip_sd(cfg, kind, num_tokens=T)
        out[kind, T] = (ipsd, load_ip_adapter(ipsd, cfg, num_tokens=T).to(dev))
    return out


def _tokens_ref(ipsd, kind, e, T=4):
    """(cond, uncond) tokens of the fp64 image projection, as fp32."""
    return image_proj_ref(ipsd, kind, e, T).float(), image_proj_ref(ipsd, kind, torch.zeros_like(e), T).float()


def _eps(unet, dev, x, t, ctx):
    with torch.no_grad():
        e = unet(x.to(dev), t.to(dev), ctx.to(dev), extra_info={})
    torch.cuda.synchronize()
    return e.cpu()


def _set(unet, ad, e, scale=1.0):
    with torch.no_grad():
        unet.set_ip_adapter(ad, ad.tokens(e), ad.uncond_tokens(e.shape[0]), scale)


# ---------------------------------------------------------------------------------------------------------------- a. tokens
@pytest.mark.parametrize("key", [("clip", 4), ("clip", 16), ("faceid", 4)])
def test_image_tokens_vs_fp64(dev, adapters, key):
    kind, T = key
    ipsd, ad = adapters[key]
    e = ip_inputs(kind, rows=3)[3]
    with torch.no_grad():
        tok, un = ad.tokens(e), ad.uncond_tokens(2)
    torch.cuda.synchronize()
    assert tok.shape == (3, T, 128) and tok.dtype == torch.float16 and un.shape == (2, T, 128)
    ref, ref0 = image_proj_ref(ipsd, kind, e, T), image_proj_ref(ipsd, kind, torch.zeros(2, e.shape[1]), T)
    err, err0 = rel_l2(tok.float().cpu().numpy(), ref.numpy()), rel_l2(un.float().cpu().numpy(), ref0.numpy())
    nonorm = rel_l2(image_proj_ref(ipsd, kind, e, T, norm=False).numpy(), ref.numpy())
    print(f"image_proj {kind} T={T}: rel-L2 vs fp64 {err:.3e} (zeros: {err0:.3e}); dropping the LayerNorm would move it by {nonorm:.3e}")
    assert err < BLOCK_TOL and err0 < BLOCK_TOL


# ---------------------------------------------------------------------------------------------------------------- b. U-Net walk
@pytest.mark.parametrize("T", [4, 16])
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_unet_with_adapter_vs_cpu_walk(dev, net, adapters, scale, T):
    unet, sd = net
    ipsd, ad = adapters["clip", T]
    cfg = motion_unet_cfg()
    x, t, ctx, e = ip_inputs("clip")
    _set(unet, ad, e, scale)
    try:
        got = _eps(unet, dev, x, t, ctx)
    finally:
        unet.set_ip_adapter(None)
    cond, uncond = _tokens_ref(ipsd, "clip", e, T)
    with torch.no_grad():
        plain = unet_forward_ip(sd, ipsd, cfg, x, t, ctx, cond, uncond, fault="no_ip")
        ref = unet_forward_ip(sd, ipsd, cfg, x, t, ctx, cond, uncond, scale=scale)
    err, moved = rel_l2(got.numpy(), ref.numpy()), rel_l2(ref.numpy(), plain.numpy())
    print(f"U-Net + IP-Adapter T={T} scale {scale}: rel-L2 vs the CPU walk {err:.3e}; the adapter moves eps by {moved:.3e}")
    assert moved > 0.05
    assert err < NET_TOL


# ---------------------------------------------------------------------------------------------------------------- c. CFG batch
def test_cond_uncond_batch_order_and_refused_batches(dev, net, adapters):
    """rows = 2: a batch of 4 runs (cond 0, cond 1, uncond, uncond), a batch of 2 the cond tokens, a batch of 3 is refused."""
    unet, sd = net
    ipsd, ad = adapters["clip", 4]
    cfg = motion_unet_cfg()
    x, t, ctx, e = ip_inputs("clip", rows=2, seed=57)
    cond, uncond = _tokens_ref(ipsd, "clip", e)
    _set(unet, ad, e)
    try:
        got4 = _eps(unet, dev, x, t, ctx)
        got2 = _eps(unet, dev, x[:2], t[:2], ctx[:2])
        with pytest.raises(ValueError, match=r"the batch \(3\) is neither the image tokens' rows \(2: cond\) nor twice that"):
            _eps(unet, dev, x[:3], t[:3], ctx[:3])
        assert all(m._ip_pre is None and m._kv_pre is None for m in unet._cross_attn_layers())
    finally:
        unet.set_ip_adapter(None)
    with torch.no_grad():
        ref4 = unet_forward_ip(sd, ipsd, cfg, x, t, ctx, cond, uncond)
        swapped = unet_forward_ip(sd, ipsd, cfg, x, t, ctx, cond, uncond, fault="swap_cond_uncond")
        ref2 = unet_forward_ip(sd, ipsd, cfg, x[:2], t[:2], ctx[:2], cond, uncond)
    e4, e2 = rel_l2(got4.numpy(), ref4.numpy()), rel_l2(got2.numpy(), ref2.numpy())
    print(f"[cond ; uncond] batch of 4 on 2 token rows: rel-L2 {e4:.3e} (swapped sets would differ by {rel_l2(swapped.numpy(), ref4.numpy()):.3e}); "
          f"cond-only batch of 2: {e2:.3e}")
    assert rel_l2(swapped.numpy(), ref4.numpy()) > 10 * NET_TOL
    assert e4 < NET_TOL and e2 < NET_TOL


# ---------------------------------------------------------------------------------------------------------------- d. bitwise restore
def test_unset_and_inactive_restore_the_plain_walk_bitwise(dev, net, adapters):
    unet, _ = net
    _, ad = adapters["clip", 4]
    x, t, ctx, e = ip_inputs("clip")
    plain = _eps(unet, dev, x, t, ctx)
    _set(unet, ad, e)
    try:
        on = _eps(unet, dev, x, t, ctx)
        unet.set_ip_adapter_active(False)
        off = _eps(unet, dev, x, t, ctx)
        unet.set_ip_adapter_active(True)
        on_again = _eps(unet, dev, x, t, ctx)
    finally:
        unet.set_ip_adapter(None)
    after = _eps(unet, dev, x, t, ctx)
    _set(unet, ad, e)
    try:
        reset = _eps(unet, dev, x, t, ctx)
        xg = x.to(dev).requires_grad_(True)
        with pytest.raises(NotImplementedError, match="training is not built with an IP-Adapter"):
            unet(xg, t.to(dev), ctx.to(dev), extra_info={})
        with pytest.raises(NotImplementedError, match="captured / score-rewrite path is not built with an IP-Adapter"):
            with torch.no_grad():
                unet(x.to(dev), t.to(dev), ctx.to(dev), extra_info={"normalize_cross_attn": True})
        with pytest.raises(NotImplementedError, match="capturing cross-attention activations is not built with an IP-Adapter"):
            with torch.no_grad():
                unet(x.to(dev), t.to(dev), ctx.to(dev), extra_info={"capture_ca_activations": True})
    finally:
        unet.set_ip_adapter(None)
    assert torch.equal(off, plain) and torch.equal(after, plain)
    assert torch.equal(on_again, on) and torch.equal(reset, on) and not torch.equal(on, plain)


# ---------------------------------------------------------------------------------------------------------------- e. combinations
def test_adapter_with_controlnet_vs_cpu_walk(dev, net, adapters):
    """The ControlNet's own cross-attention layers see the text only."""
    from adaface_dev_amd.ldm.modules.diffusionmodules.controlnet import load_controlnet
    unet, sd = net
    ipsd, ad = adapters["clip", 4]
    cfg = motion_unet_cfg()
    csd = synth_controlnet_sd(cfg)
    cn = load_controlnet(csd, cfg).to(dev)
    imgs = synth_control_images(2, 64, 64)
    x, t, ctx, e = ip_inputs("clip")
    cond, uncond = _tokens_ref(ipsd, "clip", e)
    with torch.no_grad():
        hint = cn.hint_features(imgs.to(dev))
    unet.set_control(cn, hint, 1.0)
    _set(unet, ad, e)
    try:
        got = _eps(unet, dev, x, t, ctx)
    finally:
        unet.set_control(None)
        unet.set_ip_adapter(None)
    with torch.no_grad():
        ref = unet_forward_ip(sd, ipsd, cfg, x, t, ctx, cond, uncond, csd=csd, images_u8=imgs)
        no_ip = unet_forward_ip(sd, ipsd, cfg, x, t, ctx, cond, uncond, csd=csd, images_u8=imgs, fault="no_ip")
        no_control = unet_forward_ip(sd, ipsd, cfg, x, t, ctx, cond, uncond)
    err = rel_l2(got.numpy(), ref.numpy())
    print(f"U-Net + IP-Adapter + ControlNet: rel-L2 vs the CPU walk {err:.3e}; without the adapter the walk differs by "
          f"{rel_l2(no_ip.numpy(), ref.numpy()):.3e}, without the control by {rel_l2(no_control.numpy(), ref.numpy()):.3e}")
    assert rel_l2(no_ip.numpy(), ref.numpy()) > 0.05 and rel_l2(no_control.numpy(), ref.numpy()) > 0.05
    assert err < NET_TOL


def test_adapter_with_motion_module_vs_cpu_walk(dev, net, adapters):
    """2 videos of 4 frames as (cond video, uncond video): 4 token rows, one per frame."""
    from adaface_dev_amd.ldm.modules.motion_module import MotionModule
    unet, sd = net
    ipsd, ad = adapters["clip", 4]
    cfg = motion_unet_cfg()
    msd = synth_motion_sd(cfg, with_mid=True, max_len=32, seed=5)
    mm = MotionModule(msd).to(dev)
    nf = 4
    x, _, ctx, e = ip_inputs("clip", rows=nf, seed=61)
    t = torch.tensor([700, 250]).repeat_interleave(nf)
    cond, uncond = _tokens_ref(ipsd, "clip", e)
    unet.set_motion(mm, nf)
    _set(unet, ad, e)
    try:
        got = _eps(unet, dev, x, t, ctx)
    finally:
        unet.set_ip_adapter(None)
        unet.set_motion(None)
    with torch.no_grad():
        ref = unet_forward_ip(sd, ipsd, cfg, x, t, ctx, cond, uncond, msd=msd, nf=nf)
        no_ip = unet_forward_ip(sd, ipsd, cfg, x, t, ctx, cond, uncond, msd=msd, nf=nf, fault="no_ip")
        no_motion = unet_forward_ip(sd, ipsd, cfg, x, t, ctx, cond, uncond)
    err = rel_l2(got.numpy(), ref.numpy())
    print(f"U-Net + IP-Adapter + motion module F={nf}: rel-L2 vs the CPU walk {err:.3e}; without the adapter the walk differs by "
          f"{rel_l2(no_ip.numpy(), ref.numpy()):.3e}, without the motion module by {rel_l2(no_motion.numpy(), ref.numpy()):.3e}")
    assert rel_l2(no_ip.numpy(), ref.numpy()) > 0.05 and rel_l2(no_motion.numpy(), ref.numpy()) > 0.05
    assert err < NET_TOL


# ---------------------------------------------------------------------------------------------------------------- f / g. wrapper
ENC_TINY = dict(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256, patch_size=8, image_size=32)


def _lcm_lora(unet):
    from test_lcm_host import restated_targets, synth_lora
    return synth_lora(unet, restated_targets(), 8, seed=31, alpha=4, scale=0.5)


@pytest.fixture(scope="module")
def encoder(dev):
    """A ViT-H/14-style tower (erf-GELU, projection 1024) at toy width with fp16-representable weights, and its fp64 state dict."""
    from adaface_dev_amd.evaluation import vit
    m = vit.VisionTransformer(vit.clip_vision_config("ViT-H/14", **ENC_TINY))
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        for n, p in m.named_parameters():
            v = torch.randn(p.shape, generator=g) * 0.08
            if "norm" in n and n.endswith("weight"):
                v += 1.0
            p.copy_(v.half().float())
    m.eval()
    esd = VR.to_dtype(m.state_dict())
    return m.to(dev), esd


def _encode_ref_full(encoder, images):
    """The restatement on a list of uint8 images: (last hidden states, features), fp64."""
    model, esd = encoder
    c = model.config
    sc, sh = VR.scale_shift(c.mean, c.std)
    pix = torch.cat([VR.preprocess_ref(im[None], int(c.keep_aspect), c.image_size, c.image_size, {"bilinear": 0, "bicubic": 1}[c.filter], sc, sh)[0]
                     for im in images])
    return VR.vision_forward(esd, c, pix)


def _encode_ref(encoder, images):
    return _encode_ref_full(encoder, images)[1]


def _wrapper(dev, scheduler, ip_adapter=None, encoder=None, steps=4):
    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper
    from adaface_dev_amd.adaface.arc2face_models import clip_text_config
    from adaface_dev_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    cc = clip_text_config(hidden_size=128, num_attention_heads=2, num_hidden_layers=3, intermediate_size=512)
    ld = LatentDiffusion(motion_unet_cfg())
    rng.load_synth_weights(ld.model.diffusion_model, seed=63)
    kw = dict(use_lcm=True, lcm_lora_path=_lcm_lora(ld.model.diffusion_model)) if scheduler == "lcm" else dict(default_scheduler_name=scheduler)
    w = AdaFaceWrapper(pipeline_name="text2img", clip_config=cc, ldm=ld, vae=None, device=dev, num_inference_steps=steps, ip_adapter=ip_adapter,
                       ip_image_encoder=encoder, **kw)
    return w.to(dev)


def _cpu_chain(scheduler, eps2, noise, g, S):
    """The sampler's restated update (as in test_hip_controlnet.py) driving ``eps2(x, t, i)`` -> eps of the [cond ; uncond] batch.  LCM
    re-noises from seed 3."""
    from oracle import diffusion_oracle as D
    B = noise.shape[0]
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


@pytest.mark.parametrize("kind", ["faceid", "clip"])
@pytest.mark.parametrize("scheduler", ["ddim", "dpm++", "lcm"])
def test_wrapper_text2img_vs_cpu_chain(dev, net, adapters, encoder, scheduler, kind):
    """2 rows, 4 steps, CFG, latents out (vae=None), one face id / one image per row, scale 0.8: the whole window, then the window (0, 0.5) =
    steps 0 and 1 (the chain drops the adapter for the second half).  faceid: the file's LoRA is in the U-Net's weights on both sides."""
    from adaface_dev_amd import rng
    _, sd = net
    ipsd, _ = adapters[kind, 4]
    cfg = motion_unet_cfg()
    g, S, B, scale = (1.5 if scheduler == "lcm" else 4.0), 4, 2, 0.8
    w = _wrapper(dev, scheduler, ipsd, encoder[0] if kind == "clip" else None)
    if scheduler == "lcm":
        from test_lcm_host import fused_state_dict, restated_targets
        sd = fused_state_dict(sd, _lcm_lora(w.ldm.model.diffusion_model), restated_targets())
    pe = rng.synth_input("ip.pe", (1, 77, 128), seed=85)
    ne = rng.synth_input("ip.ne", (1, 77, 128), seed=86)
    noise = rng.synth_input("ip.noise", (B, 4, 8, 8), seed=87)
    if kind == "faceid":
        sd_ip = fused_unet_sd(sd, ipsd, cfg)
        e = ip_inputs("faceid", rows=B)[3]
        arg = dict(ip_adapter_face_id=3.0 * e)                   # the wrapper normalises a caller's embedding
    else:
        sd_ip = sd
        imgs = synth_control_images(B, 40, 52, seed=13)
        e = _encode_ref(encoder, list(imgs)).float()
        arg = dict(ip_adapter_image=imgs)
    cond, uncond = _tokens_ref(ipsd, kind, e)
    c2 = torch.cat([pe.repeat(B, 1, 1), ne.repeat(B, 1, 1)])
    run = lambda **kw: w(noise.to(dev), None, prompt_embeds=(pe.to(dev), ne.to(dev)), guidance_scale=g, out_image_count=B,
                         generator=torch.Generator().manual_seed(3), **kw).cpu()
    plain = run()
    for (start, end), active in (((0.0, 1.0), {0, 1, 2, 3}), ((0.0, 0.5), {0, 1})):
        out = run(ip_adapter_scale=scale, ip_guidance_start=start, ip_guidance_end=end, **arg)
        torch.cuda.synchronize()
        assert out.shape == (B, 4, 8, 8) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
        assert w.ldm.model.diffusion_model._ip is None

        def eps2(x, t, i):
            with torch.no_grad():
                return unet_forward_ip(sd_ip, ipsd, cfg, torch.cat([x, x]).float(), torch.full((2 * B,), int(t), dtype=torch.long), c2, cond, uncond,
                                       scale=scale, fault=None if i in active else "no_ip")

        ref = _cpu_chain(scheduler, eps2, noise, g, S)
        err = rel_l2(out.numpy(), ref.numpy())
        print(f"wrapper text2img ({kind}, {scheduler}, {S} steps, CFG {g}, window {start}-{end}) rel-L2 vs the CPU chain: {err:.3e}; "
              f"the adapter moves the latents by {rel_l2(out.numpy(), plain.numpy()):.3e}")
        assert rel_l2(out.numpy(), plain.numpy()) > 0.05
        assert err < CHAIN_TOL


def test_forward_without_the_arguments_is_bitwise_the_wrapper_without_an_adapter(dev, adapters, encoder):
    from adaface_dev_amd import rng
    pe = rng.synth_input("ip.pe", (1, 77, 128), seed=85).to(dev)
    ne = rng.synth_input("ip.ne", (1, 77, 128), seed=86).to(dev)
    noise = rng.synth_input("ip.noise", (2, 4, 8, 8), seed=87).to(dev)
    run = lambda w: w(noise, None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=2)
    bare = run(_wrapper(dev, "ddim", steps=2))
    assert torch.equal(run(_wrapper(dev, "ddim", adapters["clip", 4][0], encoder[0], steps=2)), bare)
    wf = _wrapper(dev, "ddim", adapters["faceid", 4][0], steps=2)
    assert not torch.equal(run(wf), bare)                        # the FaceID LoRA lives in the weights while the adapter is loaded
    wf.unload_ip_adapter()
    assert torch.equal(run(wf), bare)


# ---------------------------------------------------------------------------------------------------------------- h. full-width block
def test_full_width_block_with_image_tokens(dev):
    """One SpatialTransformer at C = 320, N = 4096, B = 2, context 768: plain, the block takes the one-launch routes; with image tokens its attn2
    runs split and matches the fp64 restatement; without them again it is bitwise what it was."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.modules import attention as A
    C, B, H, T, ctx_dim, scale = 320, 2, 64, 4, 768, 0.7
    st = A.SpatialTransformer(C, 8, 40, context_dim=ctx_dim)
    rng.load_synth_weights(st, seed=71)
    sd = {k: v.detach().clone().double() for k, v in st.state_dict().items()}
    st = st.to(dev).eval()
    block = st.transformer_blocks[0]
    x = rng.synth_input("ip.blk.x", (B, C, H, H), seed=72)
    ctx = rng.synth_input("ip.blk.ctx", (B, 77, ctx_dim), seed=73)
    tokens = rng.synth_input("ip.blk.tok", (B, T, ctx_dim), seed=74)
    wk, wv = rng.synth_tensor("ip.blk.to_k_ip.weight", (C, ctx_dim), 75), 4.0 * rng.synth_tensor("ip.blk.to_v_ip.weight", (C, ctx_dim), 76)
    assert block.plan(C, B, H * H, ctx).xattn != "split"

    def run():
        with torch.no_grad():
            y = st(x.to(dev), ctx.to(dev))
        torch.cuda.synchronize()
        return y.cpu()

    before = run()
    kv = torch.cat([tokens.to(dev) @ wk.to(dev).t(), tokens.to(dev) @ wv.to(dev).t()], -1).to(torch.float16)      # [B, T, 2 C]: both read as slices
    block.attn2._ip_pre = (kv[:, :, :C], kv[:, :, C:], scale)
    try:
        assert block.plan(C, B, H * H, ctx).xattn == "split"
        with_ip = run()
    finally:
        block.attn2._ip_pre = None
    after = run()
    assert torch.equal(after, before)
    with torch.no_grad():
        ref = ip_spatial_transformer(sd, "", x.double(), ctx.double(), 8, wk.double(), wv.double(), tokens.double(), scale)
        plain = ip_spatial_transformer(sd, "", x.double(), ctx.double(), 8, wk.double(), wv.double(), tokens.double(), 0.0)
    err, err0 = rel_l2(with_ip.double().numpy(), ref.numpy()), rel_l2(before.double().numpy(), plain.numpy())
    moved = rel_l2(ref.numpy(), plain.numpy())
    print(f"C = 320 block, N = 4096, B = 2: with image tokens rel-L2 vs fp64 {err:.3e} (plain: {err0:.3e}); the tokens move the output by {moved:.3e}")
    assert moved > 10 * BLOCK_TOL
    assert err < BLOCK_TOL


# ---------------------------------------------------------------------------------------------------------------- i. ViT-H/14
def test_vit_h14_at_reduced_depth_vs_restatement(dev):
    """ViT-H/14 as the table has it (width 1280, 16 heads of 80, MLP 5120, erf-GELU, projection 1024, 224 / 14) with 2 of its 32 layers."""
    from adaface_dev_amd.evaluation import vit
    c = vit.clip_vision_config("ViT-H/14", num_hidden_layers=2)
    assert (c.hidden_size, c.num_attention_heads, c.intermediate_size, c.hidden_act, c.projection_dim, c.patch_size, c.image_size) == \
        (1280, 16, 5120, "gelu", 1024, 14, 224)
    assert vit.clip_vision_config("ViT-H/14").num_hidden_layers == 32
    m = vit.VisionTransformer(c)
    g = torch.Generator().manual_seed(19)
    with torch.no_grad():
        for n, p in m.named_parameters():
            fan_in = p[0].numel() if p.dim() > 1 else 1
            v = torch.randn(p.shape, generator=g) * (0.9 * fan_in ** -0.5 if p.dim() > 1 else 0.05)
            if "norm" in n and n.endswith("weight"):
                v += 1.0
            p.copy_(v.half().float())
    m.eval()
    esd = VR.to_dtype(m.state_dict())
    m = m.to(dev)
    gi = torch.Generator().manual_seed(23)
    img = torch.randint(0, 256, (250, 300, 3), generator=gi, dtype=torch.int64).to(torch.uint8)
    feats, last = m.forward_u8(img[None].to(dev), return_hidden=True)
    torch.cuda.synchronize()
    ref_last, ref_feats = _encode_ref_full((m, esd), [img])
    e_last, e_feat = VR.rel_l2(last.cpu(), ref_last), VR.rel_l2(feats.cpu(), ref_feats)
    print(f"ViT-H/14, 2 layers: last hidden rel-L2 {e_last:.3e}, image_embeds {e_feat:.3e}")
    assert tuple(last.shape) == (1, 257, 1280) and tuple(feats.shape) == (1, 1024)
    assert e_last < FEAT_BOUND and e_feat < FEAT_BOUND

