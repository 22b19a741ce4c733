"""High-resolution text2img on a real MI355X (`pytest -m gpu`): the fused latent-upscale + q_sample kernel
(af_latent_resize_q_sample) against torch's F.interpolate in fp64 on the CPU, LatentDiffusion.hires_latents' draw order, and
AdaFaceWrapper.forward(hires_size=...) against the CPU oracle at reduced width, under each sampler and at SD-1.5 size
(INTEGRATION.md "High-resolution text2img")."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from test_hip_img2img import _unet_cfg
from test_hires_host import MODES, SHAPES
from test_lcm_host import restated_targets, synth_lora
from test_vae_oracle import VAE_SMALL

pytestmark = pytest.mark.gpu

SA, SB = 0.8123, 0.5834
MODE_ID = {"bilinear": 0, "bicubic": 1}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- kernel
_CASES = {}


def _case(shape, mode, with_noise):
    """(x, noise, fp64 reference, bound) of one case, computed once on the CPU.  The reference is F.interpolate in fp64 followed by
    sa r + sb n in fp64; e_ref is the error of torch's own fp32 CPU result against it, and the bound 4 e_ref + 2^-22 max|reference|
    leaves room for another summation order.  Nothing here comes from the kernel."""
    key = (shape, mode, with_noise)
    if key not in _CASES:
        from adaface_dev_amd import rng
        P, h, w, H, W = shape
        x = rng.synth_input("hires.x", (1, P, h, w), seed=h * 100 + W)
        n = rng.synth_input("hires.n", (1, P, H, W), seed=h * 100 + W + 1) if with_noise else None
        r64 = F.interpolate(x.double(), size=(H, W), mode=mode, align_corners=False)
        r32 = F.interpolate(x, size=(H, W), mode=mode, align_corners=False)
        ref = SA * r64 + SB * n.double() if with_noise else r64
        own = SA * r32 + SB * n if with_noise else r32
        e_ref = float((own.double() - ref).abs().max())
        _CASES[key] = (x, n, ref, 4.0 * e_ref + 2.0 ** -22 * float(ref.abs().max()))
    return _CASES[key]


def _launch(dev, x, n, H, W, mode, out_offset=0):
    """The C entry point itself; out_offset floats past a 16-byte boundary for the output."""
    from adaface_dev_amd import _lib
    _, P, h, w = x.shape
    xd = x.contiguous().to(dev)
    nd = None if n is None else n.contiguous().to(dev)
    buf = torch.empty(P * H * W + out_offset, dtype=torch.float32, device=dev)
    out = buf[out_offset:]
    assert out.data_ptr() % 16 == 4 * out_offset
    rc = _lib.lib().af_latent_resize_q_sample(xd.data_ptr(), None if nd is None else nd.data_ptr(), out.data_ptr(), P, h, w, H, W,
                                              MODE_ID[mode], SA, SB, None)
    assert rc == 0, _lib.lib().af_last_error()
    torch.cuda.synchronize()
    return out.view(1, P, H, W).cpu()


@pytest.mark.parametrize("with_noise", [True, False], ids=["noise", "null"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES + ["offset"], ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_latent_resize_q_sample_vs_torch_fp64(dev, shape, mode, with_noise):
    """Absolute error per element against the fp64 reference, bound 4 e_ref + 2^-22 max|reference| (see _case).  "offset" is the
    8x8 -> 16x24 case with the output 4 bytes past a 16-byte boundary: W % 4 == 0 on the one-element form, which must also be
    bitwise the 16-byte form's output.  Two launches on the same inputs are bitwise equal.
    Measured on MI355X: not yet (the largest error over the cases goes here)."""
    offset = shape == "offset"
    shape = SHAPES[0] if offset else shape
    x, n, ref, bound = _case(shape, mode, with_noise)
    H, W = shape[3:]
    out = _launch(dev, x, n, H, W, mode, out_offset=1 if offset else 0)
    err = float((out.double() - ref).abs().max())
    print(f"latent_resize_q_sample {shape}{' +4B' if offset else ''} {mode} noise={with_noise}: max abs err {err:.3e}, bound {bound:.3e}")
    assert bool(torch.isfinite(out).all()) and err <= bound
    assert torch.equal(out, _launch(dev, x, n, H, W, mode, out_offset=1 if offset else 0))
    if offset:
        assert torch.equal(out, _launch(dev, x, n, H, W, mode))


@pytest.mark.parametrize("mode", MODES)
def test_identity_size_returns_the_input(dev, mode):
    """h x w -> h x w without noise: the weights at t = 0 are exactly (1, 0) and (0, 1, 0, 0)."""
    x, _, _, _ = _case(SHAPES[4], mode, False)
    assert SHAPES[4][1:3] == SHAPES[4][3:]
    assert torch.equal(_launch(dev, x, None, *SHAPES[4][3:], mode), x)


def test_latent_resize_q_sample_refusals(dev):
    """Every refusal returns AF_E_BADARG and sets af_last_error.  All buffers are real and large enough for the call as made, the 2^31
    cases included (8 GiB, not written by the test), so a missed check could not reach memory that is not the test's."""
    from adaface_dev_amd import _lib, ops
    L = _lib.lib()
    x = torch.zeros(4, 8, 8, device=dev)
    n = torch.zeros(4, 16, 16, device=dev)
    out = torch.zeros(4, 16, 16, device=dev)
    p = lambda t: t.data_ptr()

    def refused(*args):
        rc = L.af_latent_resize_q_sample(*args, None)
        return rc == _lib.AF_E_BADARG and b"af_latent_resize_q_sample" in L.af_last_error()

    good = [p(x), p(n), p(out), 4, 8, 8, 16, 16, 0, 0.5, 0.5]
    assert L.af_latent_resize_q_sample(*good, None) == 0
    assert refused(None, *good[1:])
    assert refused(*good[:2], None, *good[3:])
    for i in range(3, 8):                                   # P, h, w, H, W
        for bad in (0, -1):
            assert refused(*good[:i], bad, *good[i + 1:])
    for mode in (-1, 2):
        assert refused(*good[:8], mode, *good[9:])
    big = torch.empty(2 ** 33, dtype=torch.uint8, device=dev)          # 2^31 floats
    small = torch.zeros(2 ** 15, device=dev)
    assert refused(p(small), None, p(big), 2 ** 15, 1, 1, 256, 256, 0, 1.0, 0.0)        # P H W = 2^31
    assert refused(p(big), None, p(small), 2 ** 15, 256, 256, 1, 1, 1, 1.0, 0.0)        # P h w = 2^31
    del big
    torch.cuda.synchronize()
    xd = x.view(1, 4, 8, 8)
    with pytest.raises(RuntimeError, match="mode"):
        ops.latent_resize_q_sample(xd, (16, 16), "nearest")
    with pytest.raises(RuntimeError, match="noise"):
        ops.latent_resize_q_sample(xd, (16, 16), noise=torch.zeros(1, 4, 16, 8, device=dev))
    with pytest.raises(RuntimeError, match="contiguous fp32"):
        ops.latent_resize_q_sample(xd.half(), (16, 16))
    with pytest.raises(RuntimeError, match="contiguous fp32"):
        ops.latent_resize_q_sample(xd.transpose(2, 3), (16, 16))
    with pytest.raises(RuntimeError, match="size_hw"):
        ops.latent_resize_q_sample(xd, (0, 16))


# ---------------------------------------------------------------------------------------------------------------- model layer
def _small_ldm(seed=63):
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    ld = LatentDiffusion(_unet_cfg())
    rng.load_synth_weights(ld.model.diffusion_model, seed=seed)
    return ld


def _expected_hires(ld, lat, size_hw, t_first, n_hr, mode):
    import math
    from adaface_dev_amd import ops
    ac = float(ld.alphas_cumprod[t_first].double())
    return ops.latent_resize_q_sample(lat, size_hw, mode, n_hr.to(lat.device), math.sqrt(ac), math.sqrt(1.0 - ac))


@pytest.mark.parametrize("mode", MODES)
def test_hires_latents_draws_one_randn(dev, mode):
    """Under a seeded CPU generator the result is the kernel's on the generator's next randn of the output's shape, with (sa, sb) of
    t_first from the fp64 schedule."""
    from adaface_dev_amd import rng
    ld = _small_ldm().to(dev)
    lat = rng.synth_input("hires.lat", (3, 4, 16, 16), seed=5).to(dev)
    x_t = ld.hires_latents(lat, (16, 24), 251, generator=torch.Generator().manual_seed(7), mode=mode)
    n_hr = torch.randn((3, 4, 16, 24), generator=torch.Generator().manual_seed(7))
    assert x_t.shape == (3, 4, 16, 24) and x_t.dtype == torch.float32
    assert torch.equal(x_t, _expected_hires(ld, lat, (16, 24), 251, n_hr, mode))
    assert not torch.equal(x_t, ld.hires_latents(lat, (16, 24), 251, generator=torch.Generator().manual_seed(8), mode=mode))


def test_hires_latents_follows_the_lcm_draws(dev):
    """An LCM first pass of 4 steps draws its re-noising 3 times from the generator; n_hr is draw 4."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.models.diffusion.lcm import LCMSampler
    ld = _small_ldm().to(dev)
    B = 2
    c = (rng.synth_input("hires.c", (B, 77, 128), seed=80).to(dev), [""] * B, {})
    x_T = rng.synth_input("hires.xT", (B, 4, 16, 16), seed=82).to(dev)
    g = torch.Generator().manual_seed(11)
    lat, _ = LCMSampler(ld).sample(4, B, (4, 16, 16), conditioning=c, x_T=x_T, guidance_scale=1.0, generator=g)
    x_t = ld.hires_latents(lat, (24, 16), 499, generator=g)
    g2 = torch.Generator().manual_seed(11)
    for _ in range(3):
        torch.randn((B, 4, 16, 16), generator=g2)
    n_hr = torch.randn((B, 4, 24, 16), generator=g2)
    assert torch.equal(x_t, _expected_hires(ld, lat, (24, 16), 499, n_hr, "bilinear"))


# ---------------------------------------------------------------------------------------------------------------- wrapper
def _small_wrapper(dev, steps, with_vae=True, **kw):
    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper
    from adaface_dev_amd.adaface.arc2face_models import clip_text_config
    cc = clip_text_config(hidden_size=128, num_attention_heads=2, num_hidden_layers=3, intermediate_size=512)
    ld = _small_ldm()
    ae = None
    if with_vae:
        ae = ld.instantiate_first_stage(dict(VAE_SMALL, double_z=True))
        with torch.no_grad():
            for n, p in ae.named_parameters():
                p.copy_(rng.synth_tensor(n, p.shape, seed=92))
    if kw.get("use_lcm"):
        ld.to(dev)
        kw["lcm_lora_path"] = synth_lora(ld.model.diffusion_model, restated_targets(), 4, seed=31, alpha=4, scale=0.5)
    w = AdaFaceWrapper(pipeline_name="text2img", clip_config=cc, ldm=ld, vae=ae, device=dev, num_inference_steps=steps, **kw)
    return w.to(dev), ae


def _oracle_ddim_steps(sd, x, c, u, S, n, g):
    """The last n steps of the S-step DDIM schedule with CFG g from the oracle pieces on the CPU."""
    from oracle import diffusion_oracle as D
    from oracle import unet_oracle as O
    tabs = D.register_schedule(D.make_beta_schedule_linear())
    ts = D.make_ddim_timesteps(S)
    _, a, ap = D.make_ddim_sampling_parameters(tabs["alphas_cumprod"], ts)
    scales = D.guide_scale_sequence(n, g)
    B = x.shape[0]
    for i, index in enumerate(range(n - 1, -1, -1)):
        tt = torch.full((2 * B,), int(ts[index]), dtype=torch.long)
        with torch.no_grad():
            e2 = O.unet_forward(sd, _unet_cfg(), torch.cat([x, x]), tt, torch.cat([c, u]), {})
        x, _ = D.ddim_update(x, D.cfg_combine(e2[:B], e2[B:], scales[i]), float(a[index]), float(ap[index]))
    return x, int(ts[n - 1])


def test_wrapper_hires_vs_oracle_reduced_width(dev):
    """DDIM, 4 steps at 128 x 128, CFG 4, 3 outputs, then bicubic to 192 x 128 and strength 0.5 of 4 steps (2 steps from t = 251),
    against the oracle U-Net driving the 4 + 2 steps on the CPU with F.interpolate(bicubic) in fp32 and n_hr redrawn from the seed
    between them.  Bound: the project's 3.8e-3 rel-L2 for a 4-step chain at this width; this chain has 6 steps, so if the measured
    error is above that the bound is twice the measured value, at most 7.6e-3.
    Measured on MI355X: not yet."""
    from adaface_dev_amd import rng
    from oracle import diffusion_oracle as D
    w, ae = _small_wrapper(dev, 4)
    sd = {k: v.detach().cpu().clone() for k, v in w.ldm.model.diffusion_model.state_dict().items()}
    pe = rng.synth_input("hires.pe", (1, 77, 128), seed=85).to(dev)
    ne = rng.synth_input("hires.ne", (1, 77, 128), seed=86).to(dev)
    noise = rng.synth_input("hires.noise", (3, 4, 16, 16), seed=87)
    lat = []
    orig = ae.decode

    def decode_spy(zz):
        lat.append(zz)
        return orig(zz)

    ae.decode = decode_spy
    try:
        out = w(noise.to(dev), None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=3,
                generator=torch.Generator().manual_seed(7), hires_size=(192, 128), hires_strength=0.5, hires_upscaler="bicubic")
    finally:
        del ae.decode
    assert len(out) == 3 and all(im.size == (192, 128) for im in out)
    assert len(lat) == 1 and lat[0].shape == (3, 4, 16, 24)
    c, u = pe.cpu().repeat(3, 1, 1), ne.cpu().repeat(3, 1, 1)
    x, _ = _oracle_ddim_steps(sd, noise, c, u, 4, 4, 4.0)
    r = F.interpolate(x, size=(16, 24), mode="bicubic", align_corners=False)
    n_hr = torch.randn((3, 4, 16, 24), generator=torch.Generator().manual_seed(7))
    tabs = D.register_schedule(D.make_beta_schedule_linear())
    ac = float(np.asarray(tabs["alphas_cumprod"], dtype=np.float64)[251])
    x_t = (np.sqrt(ac) * r.double() + np.sqrt(1.0 - ac) * n_hr.double()).float()
    x, t_first = _oracle_ddim_steps(sd, x_t, c, u, 4, 2, 4.0)
    assert t_first == 251
    err = rel_l2((lat[0].cpu() * 0.18215).numpy(), x.numpy())
    print(f"hires wrapper (DDIM 4 steps, bicubic 16x16 -> 16x24, 2 steps, CFG 4) rel-L2 vs oracle: {err:.3e}")
    assert err < 3.8e-3


@pytest.mark.parametrize("name", ["dpm++", "lcm"])
def test_wrapper_hires_samplers(dev, name):
    """dpm++ (6 steps, then strength 0.5 of 4) and LCM (rank-4 LoRA, g = 1.5, 4 steps, then strength 0.5 of 4) run the two passes to
    finite latents of the hires shape; the U-Net sees timesteps(S) followed by timesteps(S2)[-n2:]."""
    from adaface_dev_amd import rng
    kw = dict(use_lcm=True) if name == "lcm" else dict(default_scheduler_name="dpm++")
    S, S2, g = (4, 4, 1.5) if name == "lcm" else (6, 4, 4.0)
    w, _ = _small_wrapper(dev, S, with_vae=False, **kw)
    pe = rng.synth_input("hires.pe", (1, 77, 128), seed=85).to(dev)
    ne = rng.synth_input("hires.ne", (1, 77, 128), seed=86).to(dev)
    noise = rng.synth_input("hires.noise", (2, 4, 16, 16), seed=88).to(dev)
    calls = []
    orig = w.ldm.apply_model

    def spy(x, t, c, **k):
        calls.append((int(t[0]), tuple(x.shape[2:])))
        return orig(x, t, c, **k)

    w.ldm.apply_model = spy
    try:
        out = w(noise, None, prompt_embeds=(pe, ne), guidance_scale=g, out_image_count=2, generator=torch.Generator().manual_seed(3),
                hires_size=(128, 192), hires_strength=0.5, hires_steps=S2)
    finally:
        del w.ldm.apply_model
    sampler = w._sampler()
    n2, _ = sampler.img2img_steps(S2, 0.5)
    want = [(int(t), (16, 16)) for t in sampler.timesteps(S)] + [(int(t), (24, 16)) for t in sampler.timesteps(S2)[-n2:]]
    assert n2 == 2 and calls == want
    assert out.shape == (2, 4, 24, 16) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())


def test_wrapper_hires_sd15_size_smoke(dev):
    """SD-1.5 U-Net and the full VAE (synthetic weights), 2 outputs, dpm++ at 8 steps, 512 x 512 -> 768 x 512 at strength 0.5: the U-Net
    runs 8 + 4 times, 2 finite images of 768 x 512 come back."""
    from adaface_dev_amd import SD15_UNET_CONFIG, rng
    from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper
    from adaface_dev_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    ld = LatentDiffusion(SD15_UNET_CONFIG)
    ae = ld.instantiate_first_stage()
    with torch.no_grad():
        for n, p in ae.named_parameters():
            p.copy_(rng.synth_tensor(n, p.shape, seed=90))
    w = AdaFaceWrapper(pipeline_name="text2img", default_scheduler_name="dpm++", ldm=ld, vae=ae, device=dev, num_inference_steps=8)
    rng.load_synth_weights(w.ldm.model.diffusion_model, seed=0)
    w.ldm.to(dev)
    pe = rng.synth_input("i2i.pe768", (1, 77, 768), seed=72).to(dev)
    ne = rng.synth_input("i2i.ne768", (1, 77, 768), seed=73).to(dev)
    noise = rng.synth_input("hires.noise512", (2, 4, 64, 64), seed=89).to(dev)
    calls, lat = [], []
    orig_apply, orig_decode = w.ldm.apply_model, ae.decode

    def apply_spy(x, t, c, **kw):
        calls.append(tuple(x.shape[2:]))
        return orig_apply(x, t, c, **kw)

    def decode_spy(z):
        lat.append(z)
        return orig_decode(z)

    w.ldm.apply_model, ae.decode = apply_spy, decode_spy
    try:
        imgs = w(noise, None, prompt_embeds=(pe, ne), guidance_scale=6.0, out_image_count=2, generator=torch.Generator().manual_seed(1),
                 hires_size=(768, 512), hires_strength=0.5)
    finally:
        del w.ldm.apply_model, ae.decode
    assert calls == [(64, 64)] * 8 + [(64, 96)] * 4
    assert len(imgs) == 2 and all(im.size == (768, 512) for im in imgs)
    assert lat[0].shape == (2, 4, 64, 96) and bool(torch.isfinite(lat[0]).all())
