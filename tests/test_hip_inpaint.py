"""Inpainting on a real MI355X (`pytest -m gpu`): the three fused step kernels with the mask blend as their tail
(af_cfg_{ddim,dpmpp,lcm}_inpaint_step) against the plain step kernels and an fp64 restatement of the blend, Sampler.sample_inpaint
against sample_img2img / sample for an all-ones mask and against the image latents for an all-zeros mask, and
AdaFaceWrapper(pipeline_name="inpaint") against the CPU oracle at reduced width and at SD-1.5 size (INTEGRATION.md "Inpainting")."""
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import rel_l2
from test_hip_img2img import _pil, _small_ldm, _unet_cfg
from test_vae_oracle import VAE_SMALL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- kernels
def _on(dev, t, offset):
    """t on the device, contiguous; offset 1 places it one float past a 16-byte boundary (the scalar form)."""
    if not offset:
        return t.contiguous().to(dev)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    buf[1:] = t.reshape(-1).to(dev)
    return buf[1:].view(t.shape)


def _step(kind, dev, e2, x, xb, xp, nz, has_uncond, blend):
    """One step of `kind` through ops (the plain kernel when blend is None); returns (x_next, x0 output)."""
    from adaface_dev_amd import ops
    g = 3.5
    if kind == "ddim":
        return ops.cfg_ddim_step(e2, x, g, 0.45, 0.62, has_uncond, blend=blend)
    if kind.startswith("dpmpp"):
        c1 = 0.37 if kind == "dpmpp_prev" else 0.0
        return ops.cfg_dpmpp_step(e2, x, xb, xp if c1 else None, g, 0.71, 0.70, 0.83, 0.29, c1, has_uncond, blend=blend)
    if kind == "lcm_noise":
        return ops.cfg_lcm_step(e2, x, nz, g, 0.73, 0.68, 0.97, 0.04, 0.86, 0.51, has_uncond, blend=blend)
    return ops.cfg_lcm_step(e2, x, None, g, 0.73, 0.68, 0.97, 0.04, has_uncond=has_uncond, blend=blend)


@pytest.mark.parametrize("kind", ["ddim", "dpmpp_prev", "dpmpp", "lcm_noise", "lcm"])
@pytest.mark.parametrize("has_uncond", [True, False])
@pytest.mark.parametrize("layout", ["scalar_hw", "vector", "offset"])
@pytest.mark.parametrize("bcast", [(1, 1), (3, 3), (1, 3), (3, 1)])
@pytest.mark.parametrize("last", [False, True])
def test_inpaint_step_kernels(dev, kind, has_uncond, layout, bcast, last):
    """x_next is the plain kernel's output bit for bit where the mask is 1 and the fp32 known latent where it is 0 (fma(sb, noise,
    sa z) rounded once from fp64, or z on the last step); the x0 output is the plain kernel's everywhere.  Layouts: hw = 15 (scalar,
    hw % 4 != 0), hw = 48 aligned (16-byte form), hw = 48 with every tensor one float off alignment (scalar).  The offset layout also
    runs the same data aligned, and both outputs equal the offset run's bit for bit: with the blend (scalar against 16-byte form)
    and without it (DPM-Solver++ and LCM scalar against 16-byte; the plain DDIM step runs scalar either way)."""
    from adaface_dev_amd import ops
    B, (B_img, B_mask) = 3, bcast
    h, w = (3, 5) if layout == "scalar_hw" else (6, 8)
    off = layout == "offset"
    g = torch.Generator().manual_seed(zlib.crc32(repr((kind, has_uncond, layout, bcast, last)).encode()))
    shp = (B, 4, h, w)
    e2 = torch.randn((2 * B if has_uncond else B,) + shp[1:], generator=g)
    x, xb, xp, nz, n_fwd = (torch.randn(shp, generator=g) for _ in range(5))
    z = torch.randn((B_img, 4, h, w), generator=g)
    m = (torch.rand((B_mask, 1, h, w), generator=g) < 0.5).float()
    m.view(-1)[0], m.view(-1)[-1] = 1.0, 0.0
    sa, sb = 0.8123, 0.5834
    D = lambda t: _on(dev, t, off)
    args = (D(e2), D(x), D(xb), D(xp), D(nz))
    blend = ops.InpaintBlend(D(z), None if last else D(n_fwd), D(m), sa, sb)
    y, x0 = _step(kind, dev, *args, has_uncond, blend)
    y_ref, x0_ref = _step(kind, dev, *args, has_uncond, None)
    if off:
        A = lambda t: _on(dev, t, False)
        args_a = (A(e2), A(x), A(xb), A(xp), A(nz))
        blend_a = ops.InpaintBlend(A(z), None if last else A(n_fwd), A(m), sa, sb)
        assert all(t.data_ptr() % 16 == 0 for t in args_a + (blend_a.z, blend_a.mask)) and args[1].data_ptr() % 16 == 4
        for (y_o, x0_o), b in (((y, x0), blend_a), ((y_ref, x0_ref), None)):
            y_a, x0_a = _step(kind, dev, *args_a, has_uncond, b)
            assert y_a.data_ptr() % 16 == 0 and x0_a.data_ptr() % 16 == 0
            assert torch.equal(y_a, y_o) and torch.equal(x0_a, x0_o)
    y, x0, y_ref, x0_ref = (t.cpu() for t in (y, x0, y_ref, x0_ref))
    zb = z[torch.arange(B) % B_img]
    mb = m[torch.arange(B) % B_mask].expand(shp).bool()
    if last:
        known = zb
    else:
        p = torch.tensor(sa, dtype=torch.float32) * zb                                  # sa z, one fp32 rounding
        known = (float(np.float32(sb)) * n_fwd.double() + p.double()).float()           # fma: one rounding of the exact sum
    assert torch.equal(x0, x0_ref)
    assert torch.equal(y[mb], y_ref[mb])
    assert torch.equal(y[~mb], known[~mb])
    assert bool(mb.any()) and bool((~mb).any())


def test_inpaint_step_refuses_bad_blend(dev):
    from adaface_dev_amd import _lib, ops
    x = torch.randn(2, 4, 4, 4, device=dev)
    e2 = torch.randn(4, 4, 4, 4, device=dev)
    z = torch.randn(1, 4, 4, 4, device=dev)
    m = torch.ones(1, 1, 4, 4, device=dev)
    with pytest.raises(RuntimeError, match="mask"):
        ops.cfg_ddim_step(e2, x, 2.0, 0.5, 0.6, True, blend=ops.InpaintBlend(z, None, torch.ones(1, 1, 4, 5, device=dev)))
    with pytest.raises(RuntimeError, match="noise"):
        ops.cfg_ddim_step(e2, x, 2.0, 0.5, 0.6, True, blend=ops.InpaintBlend(z, torch.randn(1, 4, 4, 4, device=dev), m, 0.5, 0.5))
    L = _lib.lib()
    out = torch.empty_like(x)
    p = lambda t: t.data_ptr()
    # hw that does not divide n, and a NULL mask
    assert L.af_cfg_ddim_inpaint_step(p(e2), p(x), p(out), None, x.numel(), 1, 2.0, 0.5, 0.6, p(z), None, p(m), 1, 1, 15, 0.0, 0.0,
                                      None) == _lib.AF_E_BADARG
    assert L.af_cfg_lcm_inpaint_step(p(e2), p(x), None, p(out), p(out), x.numel(), 1, 2.0, 0.5, 0.5, 1.0, 0.0, 0.0, 0.0, p(z), None,
                                     None, 1, 1, 16, 0.0, 0.0, None) == _lib.AF_E_BADARG
    assert L.af_cfg_dpmpp_inpaint_step(p(e2), p(x), p(x), None, p(out), p(out), x.numel(), 1, 2.0, 0.5, 0.5, 1.0, 0.0, 0.0, p(z),
                                       p(x), p(m), 0, 1, 16, 0.5, 0.5, None) == _lib.AF_E_BADARG
    assert L.af_vae_latents_z_q_sample(p(x), p(x), p(x), p(x), p(x), 0.18, 0.5, 0.5, p(out), None, 1, 1, 2, 2, None) == _lib.AF_E_BADARG


def test_vae_latents_z_matches_x_t(dev):
    """The encode entry point that also writes z: x_t is af_vae_latents_q_sample's bit for bit, and z is x_t at (sa, sb) = (1, 0)."""
    from adaface_dev_amd import ops
    g = torch.Generator().manual_seed(5)
    h = torch.randn(2, 8, 8, 8, generator=g).half().to(dev)
    qw, qb = (torch.randn(8, 8, generator=g) * 0.35).to(dev), (torch.randn(8, generator=g) * 0.1).to(dev)
    n_post, n_fwd = torch.randn(2, 4, 8, 8, generator=g).to(dev), torch.randn(4, 4, 8, 8, generator=g).to(dev)
    x_t, z = ops.vae_latents_q_sample(h, qw, qb, n_post, n_fwd, 0.18215, 0.6, 0.8, 4, with_z=True)
    assert torch.equal(x_t, ops.vae_latents_q_sample(h, qw, qb, n_post, n_fwd, 0.18215, 0.6, 0.8, 4))
    assert torch.equal(z, ops.vae_latents_q_sample(h, qw, qb, n_post, n_fwd[:2].contiguous(), 0.18215, 1.0, 0.0, 2))


# ---------------------------------------------------------------------------------------------------------------- samplers
SAMPLERS = {"ddim": (10, 0.6), "dpm++": (10, 0.7), "lcm": (4, 0.75)}


def _sampler(name, ld):
    from adaface_dev_amd.ldm.models.diffusion.ddim import DDIMSampler
    from adaface_dev_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from adaface_dev_amd.ldm.models.diffusion.lcm import LCMSampler
    return {"ddim": DDIMSampler, "dpm++": DPMSolverSampler, "lcm": LCMSampler}[name](ld)


@pytest.fixture(scope="module")
def small(dev):
    from adaface_dev_amd import rng
    ld = _small_ldm()
    rng.load_synth_weights(ld.model.diffusion_model, seed=63)
    ld = ld.to(dev)
    B = 3
    c = (rng.synth_input("inp.c", (B, 77, 128), seed=80).to(dev), [""] * B, {})
    u = (rng.synth_input("inp.u", (B, 77, 128), seed=81).to(dev), [""] * B, {})
    x = rng.synth_input("inp.x", (B, 4, 16, 16), seed=82).to(dev)
    z = rng.synth_input("inp.z", (1, 4, 16, 16), seed=83).to(dev)
    n_fwd = rng.synth_input("inp.n", (B, 4, 16, 16), seed=84).to(dev)
    return ld, B, c, u, x, z, n_fwd


def _gen(dev):
    return torch.Generator(device=dev).manual_seed(21)


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_all_ones_mask_is_img2img(dev, small, name):
    """Mask 1 everywhere: bitwise sample_img2img at strength < 1, and bitwise sample from x_T = n_fwd at strength 1."""
    ld, B, c, u, x, z, n_fwd = small
    S, strength = SAMPLERS[name]
    ones = torch.ones(1, 1, 16, 16, device=dev)
    kw = dict(guidance_scale=3.0, unconditional_conditioning=u)
    a, _ = _sampler(name, ld).sample_inpaint(S, strength, B, x, z, n_fwd, ones, c, generator=_gen(dev), **kw)
    b, _ = _sampler(name, ld).sample_img2img(S, strength, B, x, c, generator=_gen(dev), **kw)
    assert torch.equal(a, b)
    a, _ = _sampler(name, ld).sample_inpaint(S, 1.0, B, n_fwd, z, n_fwd, ones, c, generator=_gen(dev), **kw)
    b, _ = _sampler(name, ld).sample(S, B, (4, 16, 16), conditioning=c, x_T=n_fwd, verbose=False, generator=_gen(dev), **kw)
    assert torch.equal(a, b)


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_all_zeros_mask_returns_the_image_latents(dev, small, name):
    ld, B, c, u, x, z, n_fwd = small
    S, strength = SAMPLERS[name]
    lat, _ = _sampler(name, ld).sample_inpaint(S, strength, B, x, z, n_fwd, torch.zeros(B, 1, 16, 16, device=dev), c,
                                               guidance_scale=3.0, unconditional_conditioning=u, generator=_gen(dev))
    for j in range(B):
        assert torch.equal(lat[j], z[0])


# ---------------------------------------------------------------------------------------------------------------- wrapper
def _mask_pil(w, h):
    """White (repaint) on the left half and a block at the bottom right, black elsewhere."""
    a = np.zeros((h, w), dtype=np.uint8)
    a[:, : w // 2] = 255
    a[3 * h // 4:, 3 * w // 4:] = 200
    return Image.fromarray(a)


def test_wrapper_inpaint_vs_oracle_reduced_width(dev):
    """DDIM, S = 5, strength 0.8 (4 steps, CFG 4), one image and one mask to 3 outputs through the wrapper, against the oracle U-Net
    driving the same 4 steps on the CPU with the blend done in torch from the wrapper's own (z, n_fwd).  Bound: img2img's 3.8e-3
    rel-L2 on the final latents."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper, img2img_images_u8, inpaint_masks
    from adaface_dev_amd.adaface.arc2face_models import clip_text_config
    from adaface_dev_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    from oracle import diffusion_oracle as D
    from oracle import unet_oracle as O
    cc = clip_text_config(hidden_size=128, num_attention_heads=2, num_hidden_layers=3, intermediate_size=512)
    ld = LatentDiffusion(_unet_cfg())
    ae = ld.instantiate_first_stage(dict(VAE_SMALL, double_z=True))
    with torch.no_grad():
        for n, p in ae.named_parameters():
            p.copy_(rng.synth_tensor(n, p.shape, seed=92))
    w = AdaFaceWrapper(pipeline_name="inpaint", clip_config=cc, ldm=ld, vae=ae, device=dev, num_inference_steps=5)
    rng.load_synth_weights(w.ldm.model.diffusion_model, seed=63)
    sd = {k: v.detach().clone() for k, v in w.ldm.model.diffusion_model.state_dict().items()}
    w = w.to(dev)
    pe = rng.synth_input("inp.pe", (1, 77, 128), seed=85).to(dev)
    ne = rng.synth_input("inp.ne", (1, 77, 128), seed=86).to(dev)
    img, mask = _pil(128, 128, seed=4), _mask_pil(128, 128)
    lat = []
    orig = ae.decode

    def decode_spy(zz):
        lat.append(zz)
        return orig(zz)

    ae.decode = decode_spy
    try:
        out = w(img, None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=3, ref_img_strength=0.8,
                generator=torch.Generator().manual_seed(7), mask_image=mask)
    finally:
        del ae.decode
    assert len(out) == 3 and all(im.size == (128, 128) for im in out)
    n, t_first = 4, 601
    x, z, n_fwd = w.ldm.inpaint_latents(img2img_images_u8(img, 3).to(dev), 3, t_first, generator=torch.Generator().manual_seed(7),
                                        first_stage_model=ae)
    m = inpaint_masks(mask, 3, (128, 128))
    assert 0 < float(m.mean()) < 1
    tabs = D.register_schedule(D.make_beta_schedule_linear())
    ac = torch.from_numpy(np.asarray(tabs["alphas_cumprod"], dtype=np.float64))
    ts = D.make_ddim_timesteps(5)
    _, a, ap = D.make_ddim_sampling_parameters(tabs["alphas_cumprod"], ts)
    scales = D.guide_scale_sequence(n, 4.0)
    x, z, n_fwd = x.cpu(), z.cpu()[[0, 0, 0]], n_fwd.cpu()
    c, u = pe.cpu().repeat(3, 1, 1), ne.cpu().repeat(3, 1, 1)
    steps = list(range(n - 1, -1, -1))
    for i, index in enumerate(steps):
        tt = torch.full((6,), int(ts[index]), dtype=torch.long)
        with torch.no_grad():
            e2 = O.unet_forward(sd, _unet_cfg(), torch.cat([x, x]), tt, torch.cat([c, u]), {})
        e = D.cfg_combine(e2[:3], e2[3:], scales[i])
        x, _ = D.ddim_update(x, e, float(a[index]), float(ap[index]))
        if i < n - 1:
            t_next = int(ts[steps[i + 1]])
            known = (ac[t_next].sqrt() * z.double() + (1 - ac[t_next]).sqrt() * n_fwd.double()).float()
        else:
            known = z
        x = m * x + (1 - m) * known
    err = rel_l2((lat[0].cpu() * 0.18215).numpy(), x.numpy())
    print(f"inpaint wrapper (DDIM S=5, strength 0.8, CFG 4) rel-L2 vs oracle: {err:.3e}")
    assert err < 3.8e-3
    keep = (m == 0).expand(3, 4, 16, 16)
    assert torch.equal(lat[0].cpu()[keep], (z.to(dev) / 0.18215).cpu()[keep])     # the known region ends as z exactly


def test_wrapper_inpaint_sd15_size_smoke(dev):
    """SD-1.5 U-Net and the full VAE (synthetic weights), 512 x 512, 4 outputs, strength 1.0, 20 dpm++ steps: finite latents whose
    known region is the image latents bit for bit."""
    from adaface_dev_amd import rng
    from adaface_dev_amd import SD15_UNET_CONFIG
    from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper, inpaint_masks
    from adaface_dev_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    ld = LatentDiffusion(SD15_UNET_CONFIG)
    ae = ld.instantiate_first_stage()
    with torch.no_grad():
        for n, p in ae.named_parameters():
            p.copy_(rng.synth_tensor(n, p.shape, seed=90))
    w = AdaFaceWrapper(pipeline_name="inpaint", default_scheduler_name="dpm++", ldm=ld, vae=ae, device=dev, num_inference_steps=20)
    rng.load_synth_weights(w.ldm.model.diffusion_model, seed=0)
    w.ldm.to(dev)
    pe = rng.synth_input("i2i.pe768", (1, 77, 768), seed=72).to(dev)
    ne = rng.synth_input("i2i.ne768", (1, 77, 768), seed=73).to(dev)
    calls, lat, enc = [], [], []
    orig_apply, orig_decode, orig_lat = w.ldm.apply_model, ae.decode, w.ldm.inpaint_latents

    def apply_spy(x, t, c, **kw):
        calls.append(int(t[0]))
        return orig_apply(x, t, c, **kw)

    def decode_spy(zz):
        lat.append(zz)
        return orig_decode(zz)

    def lat_spy(*a, **kw):
        enc.append(orig_lat(*a, **kw))
        return enc[-1]

    w.ldm.apply_model, ae.decode, w.ldm.inpaint_latents = apply_spy, decode_spy, lat_spy
    mask = _mask_pil(512, 512)
    try:
        imgs = w(_pil(512, 512, seed=9), None, prompt_embeds=(pe, ne), guidance_scale=6.0, out_image_count=4, ref_img_strength=1.0,
                 generator=torch.Generator().manual_seed(1), mask_image=mask)
    finally:
        del w.ldm.apply_model, ae.decode, w.ldm.inpaint_latents
    assert len(calls) == 20 and len(imgs) == 4 and all(im.size == (512, 512) for im in imgs)
    x_start, z, n_fwd = enc[0]
    assert x_start is n_fwd                                   # strength 1 starts from the noise itself
    out = lat[0]
    assert out.shape == (4, 4, 64, 64) and bool(torch.isfinite(out).all())
    keep = (inpaint_masks(mask, 4, (512, 512)) == 0).to(dev).expand(4, 4, 64, 64)
    assert torch.equal(out[keep], (z[[0, 0, 0, 0]] / 0.18215)[keep])               # decode gets latents / 0.18215
