"""img2img on a real MI355X (`pytest -m gpu`): the two gfx950 kernels (uint8 image -> encoder input, quant_conv + posterior sample +
q_sample), LatentDiffusion.img2img_latents against the CPU oracle, DDIMSampler.sample_img2img against the same steps driven by the
oracle, and AdaFaceWrapper(pipeline_name="img2img") end to end at reduced width and at SD-1.5 size."""
import numpy as np
import pytest
import torch
from PIL import Image

from conftest import rel_l2
from test_vae_oracle import VAE_SMALL

pytestmark = pytest.mark.gpu


def _unet_cfg():
    """The reduced-width U-Net of test_hip_clip's wrapper test (TINY_UNET_CONFIG's head dim 4 is below the attention kernels' 8)."""
    from adaface_dev_amd import TINY_UNET_CONFIG
    return dict(TINY_UNET_CONFIG, model_channels=64, context_dim=128)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("B,H,W", [(1, 512, 512), (3, 96, 64), (2, 7, 5)])
def test_image_u8_to_nhwc_f16_bit_identical(dev, B, H, W):
    from adaface_dev_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + H + W)
    img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    img[0, 0, 0] = torch.tensor([0, 255, 128], dtype=torch.uint8)
    out = ops.image_u8_to_nhwc_f16(img.to(dev))
    assert out.shape == (B, H, W, 8) and out.dtype == torch.float16
    ref = ((img.float() / 255.0) * 2.0 - 1.0).half()
    o = out.cpu()
    assert torch.equal(o[..., :3].view(torch.int16), ref.view(torch.int16))
    assert torch.equal(o[..., 3:].view(torch.int16), torch.zeros(B, H, W, 5, dtype=torch.int16))


def _latent_case(B_img, B_out, hh, ww, mode, seed):
    """Encoder output h, quant_conv (qw, qb) and the two noise tensors.  mode "clamp": logvar = h[..., 4:8] exactly (identity rows, no
    bias), drawn in [-40, 30] across both clamp bounds; mode "mixed": dense quant_conv rows for mean and logvar."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(B_img, hh, ww, 8, generator=g)
    qw = torch.randn(8, 8, generator=g) * 0.35
    qb = torch.randn(8, generator=g) * 0.1
    if mode == "clamp":
        h[..., 4:] = torch.rand(B_img, hh, ww, 4, generator=g) * 70 - 40
        qw[4:] = 0
        qw[4:, 4:] = torch.eye(4)
        qb[4:] = 0
    n_post = torch.randn(B_img, 4, hh, ww, generator=g)
    n_fwd = torch.randn(B_out, 4, hh, ww, generator=g)
    return h.half(), qw, qb, n_post, n_fwd


def _latents_ref(h, qw, qb, n_post, n_fwd, scale, sa, sb):
    """Item 4 of the img2img contract as fp32 torch ops: moments = quant_conv(h); z = scale (mean + exp(0.5 clamp(logvar)) n_post);
    output j from image j % B_img; x_t = sa z + sb n_fwd.  Also returns the magnitude of the terms each x_t is summed from."""
    B_img, B_out = h.shape[0], n_fwd.shape[0]
    x = h.float().permute(0, 3, 1, 2)
    m = torch.nn.functional.conv2d(x, qw.reshape(8, 8, 1, 1), qb)
    mean, logvar = m[:, :4], m[:, 4:].clamp(-30.0, 20.0)
    std = torch.exp(0.5 * logvar)
    z = scale * (mean + std * n_post)
    idx = torch.arange(B_out) % B_img
    x_t = sa * z[idx] + sb * n_fwd
    terms = torch.nn.functional.conv2d(x.abs().double(), qw.abs().double().reshape(8, 8, 1, 1), qb.abs().double())[:, :4]
    mag = (abs(sa) * scale * (terms + std.double() * n_post.abs().double()))[idx] + abs(sb) * n_fwd.abs().double()
    return x_t, mag


@pytest.mark.parametrize("B_img,B_out,hh,ww", [(1, 4, 64, 64), (2, 2, 12, 8), (1, 1, 7, 5), (2, 4, 8, 8)])
@pytest.mark.parametrize("mode", ["clamp", "mixed"])
def test_vae_latents_q_sample_vs_torch(dev, B_img, B_out, hh, ww, mode):
    """fp32 accuracy against the fp32 torch restatement.  Each element's error is taken relative to the magnitude of the terms it is
    summed from, |sa| scale (sum |qw h| + |qb| + std |n_post|) + |sb| |n_fwd|, with an absolute floor of 1e-6: sa z + sb n_fwd cancels
    for some elements, where the plain relative error of any fp32 evaluation is unbounded.  Bound 2e-6; measured on MI355X: 1.6e-7 ..
    2.6e-7 over these cases."""
    from adaface_dev_amd import ops
    h, qw, qb, n_post, n_fwd = _latent_case(B_img, B_out, hh, ww, mode, seed=hh * 100 + B_out)
    if mode == "clamp":
        lv = h[..., 4:].float()
        assert float(lv.min()) < -30 and float(lv.max()) > 20            # both clamp bounds are crossed
    to = lambda t: t.contiguous().to(dev)
    worst = 0.0
    for sa, sb in ((0.6, 0.8), (0.9997, 0.0292), (1.0, 0.0)):        # (1, 0): the clean latent scale (mean + std n_post)
        x_t = ops.vae_latents_q_sample(to(h), to(qw), to(qb), to(n_post), to(n_fwd), 0.18215, sa, sb, B_out)
        assert x_t.shape == (B_out, 4, hh, ww) and x_t.dtype == torch.float32
        ref, mag = _latents_ref(h, qw, qb, n_post, n_fwd, 0.18215, sa, sb)
        err = float(((x_t.cpu().double() - ref.double()).abs() / mag.clamp_min(1e-6)).max())
        worst = max(worst, err)
        assert err <= 2e-6, (sa, sb, err)
        if sb == 0.0:
            for j in range(B_out):                      # outputs of one image share its posterior sample
                assert torch.equal(x_t[j].cpu(), x_t[j % B_img].cpu())
    print(f"vae_latents_q_sample {B_img}->{B_out} {hh}x{ww} {mode}: max term-relative error {worst:.2e}")


def test_vae_latents_q_sample_refuses_uneven_batch(dev):
    from adaface_dev_amd import _lib, ops
    h, qw, qb, n_post, n_fwd = _latent_case(2, 3, 8, 8, "mixed", seed=5)
    hd, qwd, qbd, npd, nfd = (t.contiguous().to(dev) for t in (h, qw, qb, n_post, n_fwd))
    with pytest.raises(RuntimeError, match="multiple"):
        ops.vae_latents_q_sample(hd, qwd, qbd, npd, nfd, 0.18215, 0.5, 0.5, 3)
    x_t = torch.empty((3, 4, 8, 8), device=dev)
    L = _lib.lib()
    rc = L.af_vae_latents_q_sample(hd.data_ptr(), qwd.data_ptr(), qbd.data_ptr(), npd.data_ptr(), nfd.data_ptr(), 0.18215, 0.5, 0.5,
                                   x_t.data_ptr(), 2, 3, 8, 8, None)
    assert rc == _lib.AF_E_BADARG and b"multiple" in L.af_last_error()
    assert L.af_image_u8_to_nhwc_f16(None, x_t.data_ptr(), 1, 8, 8, None) == _lib.AF_E_BADARG
    assert L.af_image_u8_to_nhwc_f16(hd.data_ptr(), x_t.data_ptr(), 1, 0, 8, None) == _lib.AF_E_BADARG


# ---------------------------------------------------------------------------------------------------------------- model layer
def _small_ldm():
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    ld = LatentDiffusion(_unet_cfg())
    ae = ld.instantiate_first_stage(dict(VAE_SMALL, double_z=True))
    with torch.no_grad():
        for n, p in ae.named_parameters():
            p.copy_(rng.synth_tensor(n, p.shape, seed=92))
    return ld


@pytest.mark.parametrize("B_img,B_out,t", [(2, 4, 781), (1, 3, 1), (2, 2, 541)])
def test_img2img_latents_vs_oracle(dev, B_img, B_out, t):
    """uint8 images -> x_t on the reduced-width VAE against vae_oracle.encode + the posterior + diffusion_oracle.q_sample with the same
    noise tensors; the encoder runs once, on the B_img images.  Bound 1e-2 rel-L2 (the encoder's), on x_t and on its image part;
    measured on MI355X: 4.1e-5 .. 8.8e-4 (x_t), 8.8e-4 .. 9.3e-4 (image part)."""
    from oracle import diffusion_oracle as D
    from oracle import vae_oracle as VO
    ld = _small_ldm()
    sd = {k: v.detach().float().clone() for k, v in ld.first_stage_model.state_dict().items()}
    ld = ld.to(dev)
    enc = ld.first_stage_model.encoder
    calls = []
    orig = enc.hip

    def spy(x, mask=None):
        calls.append(tuple(x.shape))
        return orig(x, mask)

    enc.hip = spy
    try:
        img = torch.randint(0, 256, (B_img, 128, 128, 3), generator=torch.Generator().manual_seed(t), dtype=torch.uint8)
        x_t = ld.img2img_latents(img.to(dev), B_out, t, generator=torch.Generator(device=dev).manual_seed(11))
    finally:
        del enc.hip
    assert calls == [(B_img, 128, 128, 8)]
    assert x_t.shape == (B_out, 4, 16, 16) and x_t.dtype == torch.float32 and bool(torch.isfinite(x_t).all())
    g = torch.Generator(device=dev).manual_seed(11)
    n_post = torch.randn((B_img, 4, 16, 16), generator=g, device=dev).cpu()
    n_fwd = torch.randn((B_out, 4, 16, 16), generator=g, device=dev).cpu()
    x = ((img.float() / 255.0) * 2.0 - 1.0).permute(0, 3, 1, 2)
    with torch.no_grad():
        mean, logvar = VO.encode(sd, x)
    z = 0.18215 * (mean + torch.exp(0.5 * logvar) * n_post)
    tabs = D.register_schedule(D.make_beta_schedule_linear())
    ref = D.q_sample(tabs, z[torch.arange(B_out) % B_img], torch.full((B_out,), t, dtype=torch.long), n_fwd)
    err = rel_l2(x_t.cpu().numpy(), ref.numpy())
    noise_part = float(tabs["sqrt_one_minus_alphas_cumprod"][t]) * n_fwd
    err_img = rel_l2((x_t.cpu() - noise_part).numpy(), (ref - noise_part).numpy())
    print(f"img2img_latents {B_img}->{B_out} t={t}: rel-L2 {err:.2e} (x_t), {err_img:.2e} (its image part sa * z)")
    assert err < 1e-2 and err_img < 1e-2


def _oracle_img2img(sd, cfg, x_t, c, u, S, n, g):
    """The last n steps of the S-step DDIM schedule with CFG, from the oracle pieces on the CPU."""
    from oracle import diffusion_oracle as D
    from oracle import unet_oracle as O
    tabs = D.register_schedule(D.make_beta_schedule_linear())
    ts = D.make_ddim_timesteps(S)
    _, a, ap = D.make_ddim_sampling_parameters(tabs["alphas_cumprod"], ts)
    scales = D.guide_scale_sequence(n, g)
    x, B = x_t.clone(), x_t.shape[0]
    for i, index in enumerate(range(n - 1, -1, -1)):
        tt = torch.full((2 * B,), int(ts[index]), dtype=torch.long)
        with torch.no_grad():
            e2 = O.unet_forward(sd, cfg, torch.cat([x, x]), tt, torch.cat([c, u]), {})
        e = D.cfg_combine(e2[:B], e2[B:], scales[i])
        x, _ = D.ddim_update(x, e, float(a[index]), float(ap[index]))
    return x


def test_sample_img2img_vs_oracle(dev):
    """S = 10, strength 0.6: 6 steps with CFG 4 on the reduced-width U-Net against the oracle driving the same 6 steps on the CPU.
    Drift measured on MI355X: rel-L2 1.87e-3; the bound is 2x that."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.models.diffusion.ddim import DDIMSampler
    ld = _small_ldm()
    rng.load_synth_weights(ld.model.diffusion_model, seed=63)
    sd = {k: v.detach().clone() for k, v in ld.model.diffusion_model.state_dict().items()}
    ld = ld.to(dev)
    x_t = rng.synth_input("i2i.xt", (2, 4, 16, 16), seed=64)
    c = rng.synth_input("i2i.c", (2, 77, 128), seed=64)
    u = rng.synth_input("i2i.u", (2, 77, 128), seed=65)
    sampler = DDIMSampler(ld)
    assert sampler.img2img_steps(10, 0.6) == (6, 501)
    seen = []
    lat, inter = sampler.sample_img2img(10, 0.6, 2, x_t.to(dev), (c.to(dev), [""] * 2, {}), guidance_scale=4.0,
                                        unconditional_conditioning=(u.to(dev), [""] * 2, {}), callback=seen.append)
    assert seen == list(range(6)) and len(inter["x_inter"]) == 3          # x_t, after index n-1, after index 0
    ref = _oracle_img2img(sd, _unet_cfg(), x_t, c, u, 10, 6, 4.0)
    err = rel_l2(lat.cpu().numpy(), ref.numpy())
    print(f"sample_img2img (S=10, strength 0.6, 6 steps, CFG 4) rel-L2 vs oracle: {err:.3e}")
    assert err < 3.8e-3


def test_sample_img2img_full_strength_is_sample(dev):
    """Strength 1.0 runs the whole schedule: bitwise the text2img sampler started from the same latent."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.models.diffusion.ddim import DDIMSampler
    ld = _small_ldm()
    rng.load_synth_weights(ld.model.diffusion_model, seed=63)
    ld = ld.to(dev)
    x_t = rng.synth_input("i2i.xt1", (2, 4, 16, 16), seed=66).to(dev)
    c = (rng.synth_input("i2i.c1", (2, 77, 128), seed=66).to(dev), [""] * 2, {})
    u = (rng.synth_input("i2i.u1", (2, 77, 128), seed=67).to(dev), [""] * 2, {})
    a, _ = DDIMSampler(ld).sample_img2img(5, 1.0, 2, x_t, c, guidance_scale=5.0, unconditional_conditioning=u)
    b, _ = DDIMSampler(ld).sample(5, 2, (4, 16, 16), conditioning=c, x_T=x_t, verbose=False, guidance_scale=5.0,
                                  unconditional_conditioning=u)
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- wrapper
def _pil(w, h, seed):
    return Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8))


def _bytes(images):
    return [np.asarray(im).tobytes() for im in images]


def test_wrapper_img2img_end_to_end_reduced_width(dev):
    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper, img2img_images_u8
    from adaface_dev_amd.adaface.arc2face_models import clip_text_config
    from adaface_dev_amd.ldm.models.diffusion.ddim import DDIMSampler
    from adaface_dev_amd.ldm.modules.diffusionmodules.model import AutoencoderKLDecoder
    cc = clip_text_config(hidden_size=128, num_attention_heads=2, num_hidden_layers=3, intermediate_size=512)
    w = AdaFaceWrapper(pipeline_name="img2img", clip_config=cc, unet_config=_unet_cfg(), device=dev, num_inference_steps=5)
    rng.load_synth_weights(w.ldm.model.diffusion_model, seed=63)
    ae = w.ldm.instantiate_first_stage(dict(VAE_SMALL, double_z=True))
    with torch.no_grad():
        for n, p in ae.named_parameters():
            p.copy_(rng.synth_tensor(n, p.shape, seed=92))
    w.vae = ae
    w = w.to(dev)
    pe = rng.synth_input("i2i.pe", (1, 77, 128), seed=70).to(dev)
    ne = rng.synth_input("i2i.ne", (1, 77, 128), seed=71).to(dev)
    img = _pil(128, 128, seed=3)

    def run(gen, strength=0.8):
        return w(img, None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=3, ref_img_strength=strength, generator=gen)

    out = run(torch.Generator().manual_seed(7))
    assert len(out) == 3 and all(im.size == (128, 128) and im.mode == "RGB" for im in out)
    # the same thing composed by hand: img2img_latents -> sample_img2img -> decode, same seeded generator
    sampler = DDIMSampler(w.ldm)
    n, t_first = sampler.img2img_steps(5, 0.8)
    assert (n, t_first) == (4, 601)
    x_t = w.ldm.img2img_latents(img2img_images_u8(img, 3).to(dev), 3, t_first, generator=torch.Generator().manual_seed(7),
                                first_stage_model=ae)
    lat, _ = sampler.sample_img2img(5, 0.8, 3, x_t, (pe.repeat(3, 1, 1), [""] * 3, {}), guidance_scale=4.0,
                                    unconditional_conditioning=(ne.repeat(3, 1, 1), [""] * 3, {}))
    dec = ae.decode(lat / 0.18215)
    man = ((dec.float() / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
    assert _bytes(out) == [m.tobytes() for m in man]
    assert _bytes(out)[0] != _bytes(out)[1]                               # forward noise drawn per output
    # reproducible under a seeded generator, CPU or CUDA
    assert _bytes(run(torch.Generator().manual_seed(7))) == _bytes(out)
    assert _bytes(run(torch.Generator(device=dev).manual_seed(8))) == _bytes(run(torch.Generator(device=dev).manual_seed(8)))
    # strength decides how many steps run (0.3 x 5 = 1 step, 0.8 x 5 = 4 steps)
    low = run(torch.Generator().manual_seed(7), strength=0.3)
    assert all(a != b for a, b in zip(_bytes(low), _bytes(out)))
    # the img2img pipeline needs the encoder
    w.vae = AutoencoderKLDecoder(dict(VAE_SMALL)).to(dev).eval()
    with pytest.raises(ValueError, match="AutoencoderKL"):
        run(torch.Generator().manual_seed(7))


def test_wrapper_img2img_sd15_size_smoke(dev):
    """SD-1.5 U-Net and the full VAE (synthetic weights), one 512 x 512 image, 4 outputs, strength 0.8 of 50 steps: 40 U-Net calls."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper
    w = AdaFaceWrapper(pipeline_name="img2img", device=dev, num_inference_steps=50)
    rng.load_synth_weights(w.ldm.model.diffusion_model, seed=0)
    ae = w.ldm.instantiate_first_stage()
    with torch.no_grad():
        for n, p in ae.named_parameters():
            p.copy_(rng.synth_tensor(n, p.shape, seed=90))
    w.vae = ae
    w.ldm.to(dev)
    pe = rng.synth_input("i2i.pe768", (1, 77, 768), seed=72).to(dev)
    ne = rng.synth_input("i2i.ne768", (1, 77, 768), seed=73).to(dev)
    calls, lat = [], []
    orig_apply, orig_decode = w.ldm.apply_model, ae.decode

    def apply_spy(x, t, c, **kw):
        calls.append(int(t[0]))
        return orig_apply(x, t, c, **kw)

    def decode_spy(z):
        lat.append(z)
        return orig_decode(z)

    w.ldm.apply_model, ae.decode = apply_spy, decode_spy
    try:
        imgs = w(_pil(512, 512, seed=9), None, prompt_embeds=(pe, ne), guidance_scale=6.0, out_image_count=4, ref_img_strength=0.8,
                 generator=torch.Generator().manual_seed(1))
    finally:
        del w.ldm.apply_model, ae.decode
    assert len(calls) == 40 and calls[0] == 781 and calls[-1] == 1
    assert len(imgs) == 4 and all(im.size == (512, 512) for im in imgs)
    assert lat[0].shape == (4, 4, 64, 64) and bool(torch.isfinite(lat[0]).all())
