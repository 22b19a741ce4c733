"""LCM-LoRA on a real MI355X (`pytest -m gpu`): the fused guidance + LCM step kernel af_cfg_lcm_step against fp64, a LoRA fused into a
reduced-width U-Net against the CPU oracle on weights fused by this file's own name map (all 278 targets, then one family at a time:
a stale packed cache fails it), LCMSampler trajectories against oracle-driven fp64 steps, and AdaFaceWrapper(use_lcm=True)."""
import time

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import rel_l2
from test_hip_unet import GPU_TINY_CONFIG, NET_TOL
from test_lcm_host import fused_state_dict, restated_targets, synth_lora
from test_vae_oracle import VAE_SMALL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ac():
    from adaface_dev_amd import TINY_UNET_CONFIG
    from adaface_dev_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    return LatentDiffusion(dict(TINY_UNET_CONFIG)).alphas_cumprod.double().numpy()


# ---------------------------------------------------------------------------------------------------------------- kernel
def _coefs(ac, last):
    """(sqrt_a, sqrt_1ma, c_out, c_skip, sqrt_a_next, sqrt_1ma_next) of the first (999 -> 759) or last (259) step of the 4-step run."""
    from adaface_dev_amd.ldm.models.diffusion.lcm import lcm_step_coefficients, lcm_timesteps
    co = lcm_step_coefficients(ac, lcm_timesteps(4))
    return co[3][:4] + (0.0, 0.0) if last else co[0]


def _kernel_ref(ec, eu, x, nz, has_uncond, g, sa, sb, c_out, c_skip, sa_n, sb_n, last):
    """fp64 reference and the magnitude of the terms each output is summed from (relative errors are taken against it)."""
    ec, eu, x, nz = (t.double() for t in (ec, eu, x, nz))
    if has_uncond:
        e, e_mag = eu + g * (ec - eu), eu.abs() + abs(g) * (ec.abs() + eu.abs())
    else:
        e, e_mag = ec, ec.abs()
    x0 = (x - sb * e) / sa
    d = c_out * x0 + c_skip * x
    d_mag = abs(c_out) * (x.abs() + sb * e_mag) / sa + abs(c_skip) * x.abs()
    if last:
        return d, d, d_mag, d_mag
    return sa_n * d + sb_n * nz, d, sa_n * d_mag + sb_n * nz.abs(), d_mag


# fp32 evaluation of a handful of operations: bound 1e-6 of the term magnitude (8 ulp), as for af_cfg_dpmpp_step; measured on MI355X
# at most 2.2e-7
KERNEL_TOL = 1e-6


@pytest.mark.parametrize("n,offset", [(4 * 4 * 64 * 64, 0), (4 * 4 * 96 * 64, 0), (1001, 0), (4096, 1)])
@pytest.mark.parametrize("has_uncond", [True, False])
@pytest.mark.parametrize("last", [False, True])
def test_kernel_vs_fp64(dev, ac, n, offset, has_uncond, last):
    """af_cfg_lcm_step against fp64, error relative to the magnitude of the summed terms: the 16-byte path (n % 4 == 0, aligned), the
    scalar path for n = 1001 and for views one float off 16-byte alignment (offset 1), the last step with noise = NULL.  Bound 1e-6;
    measured on MI355X: 1.1e-7 .. 2.2e-7 over these cases (re-noising steps the largest)."""
    from adaface_dev_amd import ops
    g = torch.Generator().manual_seed(n + 7 * has_uncond + 3 * last)
    ec, eu, x, nz = (torch.randn(n, generator=g) for _ in range(4))
    eps2 = torch.cat([ec, eu]) if has_uncond else ec.clone()

    def dview(t):                                  # a device view that starts `offset` floats into its buffer
        buf = torch.zeros(t.numel() + offset, device=dev)
        buf[offset:] = t.to(dev)
        return buf[offset:]

    gd = 1.5
    sa, sb, c_out, c_skip, sa_n, sb_n = _coefs(ac, last)
    e_d, x_d = dview(eps2), dview(x)
    if offset:
        assert e_d.data_ptr() % 16 and x_d.data_ptr() % 16
    x_next, den = ops.cfg_lcm_step(e_d, x_d, None if last else dview(nz), gd, sa, sb, c_out, c_skip, sa_n, sb_n, has_uncond)
    assert torch.isfinite(x_next).all() and torch.isfinite(den).all()
    ref, ref_d, mag, mag_d = _kernel_ref(ec, eu, x, nz, has_uncond, gd, sa, sb, c_out, c_skip, sa_n, sb_n, last)
    err = float(((x_next.cpu().double() - ref).abs() / mag.clamp_min(1e-30)).max())
    err_d = float(((den.cpu().double() - ref_d).abs() / mag_d.clamp_min(1e-30)).max())
    print(f"cfg_lcm_step n={n} offset={offset} uncond={has_uncond} last={last}: term-relative error x_next {err:.2e}, denoised {err_d:.2e}")
    assert err < KERNEL_TOL and err_d < KERNEL_TOL
    if last:
        assert torch.equal(x_next, den)


def test_kernel_refuses_bad_arguments(dev):
    from adaface_dev_amd import _lib
    L = _lib.lib()
    n = 64
    b = [torch.zeros(2 * n, device=dev) for _ in range(5)]
    p = [t.data_ptr() for t in b]

    def call(ptrs=p, nn=n, g=1.5, sa=0.5, sb=0.8, c_out=0.9, c_skip=0.1, sa_n=0.6, sb_n=0.7):
        return L.af_cfg_lcm_step(*ptrs, nn, 1, g, sa, sb, c_out, c_skip, sa_n, sb_n, None)

    assert call() == 0
    torch.cuda.synchronize()
    for i in (0, 1, 3, 4):
        assert call(ptrs=[None if j == i else q for j, q in enumerate(p)]) == _lib.AF_E_BADARG, i
    no_noise = [None if j == 2 else q for j, q in enumerate(p)]
    assert call(ptrs=no_noise, sa_n=0.0, sb_n=0.0) == 0                  # the last step: the next coefficients are unused
    torch.cuda.synchronize()
    for kw in (dict(nn=0), dict(nn=-4), dict(sa=0.0), dict(sa=-0.5), dict(sa=1.5), dict(sb=1.0), dict(sb=-0.1),
               dict(sa_n=0.0), dict(sa_n=1.5), dict(sb_n=1.0), dict(sb_n=-0.1), dict(c_out=float("nan")),
               dict(c_skip=float("inf")), dict(g=float("nan")), dict(sa_n=float("nan")), dict(sb_n=float("-inf"))):
        assert call(**kw) == _lib.AF_E_BADARG, kw
    assert call(ptrs=no_noise, sa_n=float("nan")) == _lib.AF_E_BADARG
    assert b"af_cfg_lcm_step" in L.af_last_error()


# ---------------------------------------------------------------------------------------------------------------- fused U-Net
FAMILIES = ("attn1.to_k", "attn2.to_v", "time_emb_proj", "ff.net.0.proj", "conv_shortcut", "downsamplers.0.conv",
            "upsamplers.0.conv", "proj_in")


@pytest.fixture(scope="module")
def tiny(dev):
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    m = UNetModel(**GPU_TINY_CONFIG)
    rng.load_synth_weights(m, seed=11)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m.to(dev).eval(), sd


def test_fused_unet_vs_oracle(dev, tiny):
    """A rank-8, alpha-4 LoRA over all 278 targets fused into a U-Net whose packed caches already exist (one forward before the fuse),
    against oracle.unet_forward on the state dict fused by this file's own map; then one family at a time (scale 2), each of which must
    match the oracle and move epsilon by more than 3 NET_TOL (a stale concatenated / interleaved pack fails).  After every unfuse
    epsilon is bitwise the pre-fuse epsilon.  Measured on MI355X: 1.8e-3 .. 2.8e-3 against the oracle (ff.net.0.proj the largest;
    test_hip_unet's NET_TOL 4e-3 is the bound); every family moves epsilon by 0.24 .. 1.3."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface import sd_lora
    from oracle import unet_oracle as O
    m, sd = tiny
    x = rng.synth_input("t64.x", (2, 4, 32, 32), seed=11)
    ctx = rng.synth_input("t64.ctx", (2, 77, 64), seed=11)
    t = torch.tensor([10, 500])
    run = lambda: m(x.to(dev), t.to(dev), ctx.to(dev), extra_info={})
    with torch.no_grad():
        eps0 = run()
    targets = restated_targets()
    cases = [("all", targets, 1.0)] + [(f, {d: l for d, l in targets.items() if d.endswith(f)}, 2.0) for f in FAMILIES]
    worst = 0.0
    for name, tg, scale in cases:
        lsd = synth_lora(m, tg, 8, seed=21, alpha=4)
        saved = sd_lora.fuse_unet_lora(m, sd_lora.read_unet_lora(lsd, m), scale)
        with torch.no_grad():
            eps = run()
        ref = O.unet_forward(fused_state_dict(sd, lsd, tg, scale), GPU_TINY_CONFIG, x, t, ctx, {})
        err, moved = rel_l2(eps.cpu().numpy(), ref.numpy()), rel_l2(eps.cpu().numpy(), eps0.cpu().numpy())
        print(f"fused {name} ({len(tg)} layers): eps vs oracle {err:.2e}, moved from the unfused eps by {moved:.2e}")
        worst = max(worst, err)
        assert err < NET_TOL, name
        assert moved > 3 * NET_TOL, name
        sd_lora.unfuse_unet_lora(m, saved)
        with torch.no_grad():
            assert torch.equal(run(), eps0), name
    print(f"fused U-Net vs oracle: worst {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------- trajectory
# 2x the worst per-step value measured on MI355X (docstring of test_trajectory_vs_oracle)
TRAJ_TOL = {"denoised": 2.5e-3, "x_next": 2.4e-3, "teacher_eps": 4.5e-3}


@pytest.fixture(scope="module")
def tiny_ldm(dev):
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    ldm = LatentDiffusion(GPU_TINY_CONFIG)
    rng.load_synth_weights(ldm.model.diffusion_model, seed=12)
    sd = {k: v.detach().clone() for k, v in ldm.model.diffusion_model.state_dict().items()}
    return ldm.to(dev).eval(), sd


@pytest.mark.parametrize("guidance", [1.5, 1.0])
def test_trajectory_vs_oracle(dev, tiny_ldm, guidance):
    """LCMSampler.sample(4) on the reduced-width U-Net (synthetic weights, one image; g = 1.5 runs the (cond, uncond) batch, g = 1 the
    cond batch alone) with a seeded generator, against oracle.unet_forward driven by fp64 LCM steps with the same noise draws.  Per
    step: the denoised sample, x_next and the teacher-forced guided epsilon (the GPU U-Net on the oracle's own x_i).
    Worst step measured on MI355X (the bounds TRAJ_TOL are 2x), all at t = 999 and about level over the later steps:
        g = 1.5   denoised 1.22e-3, x_next 1.19e-3, teacher-forced eps 2.23e-3
        g = 1.0   denoised 0.89e-3, x_next 0.87e-3, teacher-forced eps 1.69e-3
    The oracle costs about 1 s of CPU per guidance value."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.models.diffusion.lcm import LCMSampler, lcm_step_coefficients, lcm_timesteps
    from oracle import unet_oracle as O
    ldm, sd = tiny_ldm
    x_T = rng.synth_input("lcm.x", (1, 4, 32, 32), seed=54)
    c = rng.synth_input("lcm.ctx", (1, 77, 64), seed=54)
    u = rng.synth_input("lcm.uctx", (1, 77, 64), seed=54)
    cd, ud = (c.to(dev), [""], {}), (u.to(dev), [""], {})
    calls = []
    orig = ldm.apply_model

    def spy(x, t, cc, **kw):
        calls.append((int(t[0]), x.shape[0]))
        return orig(x, t, cc, **kw)

    ldm.apply_model = spy
    try:
        lat, inter = LCMSampler(ldm).sample(4, 1, (4, 32, 32), conditioning=cd, x_T=x_T.to(dev), guidance_scale=guidance,
                                            unconditional_conditioning=ud, log_every_t=1, generator=torch.Generator().manual_seed(3))
    finally:
        del ldm.apply_model
    ts = lcm_timesteps(4).tolist()
    cfg = guidance > 1
    assert calls == [(t, 2 if cfg else 1) for t in ts]
    gx, gd = inter["x_inter"][1:], inter["pred_x0"][1:]
    assert len(gx) == 4 and torch.equal(gx[-1], lat) and torch.equal(gd[-1], lat)

    t0 = time.perf_counter()
    ac = ldm.alphas_cumprod.detach().double().cpu().numpy()
    gen = torch.Generator().manual_seed(3)
    x = x_T.double()
    worst = dict.fromkeys(TRAJ_TOL, 0.0)
    for i, (t, (sa, sb, c_out, c_skip, sa_n, sb_n)) in enumerate(zip(ts, lcm_step_coefficients(ac, ts))):
        with torch.no_grad():
            if cfg:
                e2 = O.unet_forward(sd, GPU_TINY_CONFIG, torch.cat([x, x]).float(), torch.tensor([t, t]), torch.cat([c, u]), {}).double()
                e = e2[1:] + guidance * (e2[:1] - e2[1:])
                xd = x.float().to(dev)
                g2 = ldm.apply_model(torch.cat([xd, xd]), torch.full((2,), t, dtype=torch.int64, device=dev),
                                     (torch.cat([cd[0], ud[0]]), ["", ""], {})).cpu().double()
                e_tf = g2[1:] + guidance * (g2[:1] - g2[1:])
            else:
                e = O.unet_forward(sd, GPU_TINY_CONFIG, x.float(), torch.tensor([t]), c, {}).double()
                e_tf = ldm.apply_model(x.float().to(dev), torch.full((1,), t, dtype=torch.int64, device=dev), cd).cpu().double()
        d = c_out * (x - sb * e) / sa + c_skip * x
        x = sa_n * d + sb_n * torch.randn(x.shape, generator=gen).double() if i < 3 else d
        errs = {"denoised": rel_l2(gd[i].cpu().numpy(), d.numpy()), "x_next": rel_l2(gx[i].cpu().numpy(), x.numpy()),
                "teacher_eps": rel_l2(e_tf.numpy(), e.numpy())}
        print(f"g = {guidance} step {i} (t = {t}): " + "  ".join(f"{k} {v:.3e}" for k, v in errs.items()))
        for k, v in errs.items():
            worst[k] = max(worst[k], v)
    print(f"g = {guidance}: oracle steps in {time.perf_counter() - t0:.1f} s; worst {worst}")
    for k, v in worst.items():
        assert v < TRAJ_TOL[k], (k, v)


# ---------------------------------------------------------------------------------------------------------------- wrapper
def _unet_cfg():
    from adaface_dev_amd import TINY_UNET_CONFIG
    return dict(TINY_UNET_CONFIG, model_channels=64, context_dim=128)


def _wrapper(dev, pipeline_name="text2img", use_lcm=True, steps=4):
    """A reduced-width wrapper on synthetic weights (seed 63); use_lcm fuses the rank-8 LoRA of _lora() at construction."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper
    from adaface_dev_amd.adaface.arc2face_models import clip_text_config
    from adaface_dev_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    cc = clip_text_config(hidden_size=128, num_attention_heads=2, num_hidden_layers=3, intermediate_size=512)
    ldm = LatentDiffusion(_unet_cfg())
    rng.load_synth_weights(ldm.model.diffusion_model, seed=63)
    ldm.to(dev)
    kw = dict(use_lcm=True, lcm_lora_path=_lora(ldm)) if use_lcm else {}
    w = AdaFaceWrapper(pipeline_name=pipeline_name, clip_config=cc, ldm=ldm, device=dev, num_inference_steps=steps, **kw)
    if pipeline_name == "img2img":
        ae = w.ldm.instantiate_first_stage(dict(VAE_SMALL, double_z=True))
        with torch.no_grad():
            for n, p in ae.named_parameters():
                p.copy_(rng.synth_tensor(n, p.shape, seed=92))
        w.vae = ae
    return w.to(dev)


def _lora(ldm):
    return synth_lora(ldm.model.diffusion_model, restated_targets(), 8, seed=31, alpha=4, scale=0.5)


def _spy_calls(ldm):
    calls = []
    orig = ldm.apply_model

    def spy(x, t, c, **kw):
        calls.append((int(t[0]), x.shape[0]))
        return orig(x, t, c, **kw)

    ldm.apply_model = spy
    return calls


def _embs(dev):
    from adaface_dev_amd import rng
    return rng.synth_input("lcm.pe", (1, 77, 128), seed=80).to(dev), rng.synth_input("lcm.ne", (1, 77, 128), seed=81).to(dev)


@pytest.mark.parametrize("guidance", [1.0, 1.5])
def test_wrapper_text2img_lcm(dev, guidance):
    """text2img with use_lcm and 4 steps: U-Net calls at 999, 759, 499, 259 on batch 3 (g = 1) or 6 (g = 1.5); bitwise
    LCMSampler.sample driven by hand with the same generator seed; another seed gives another output."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.models.diffusion.lcm import LCMSampler
    pe, ne = _embs(dev)
    noise = rng.synth_input("lcm.noise", (3, 4, 16, 16), seed=82).to(dev)
    w = _wrapper(dev)
    calls = _spy_calls(w.ldm)
    try:
        out = w(noise, None, prompt_embeds=(pe, ne), guidance_scale=guidance, out_image_count=3,
                generator=torch.Generator().manual_seed(5))
    finally:
        del w.ldm.apply_model
    assert calls == [(t, 3 if guidance <= 1 else 6) for t in (999, 759, 499, 259)]
    assert out.shape == (3, 4, 16, 16) and bool(torch.isfinite(out).all())
    ref, _ = LCMSampler(w.ldm).sample(4, 3, (4, 16, 16), conditioning=(pe.repeat(3, 1, 1), [""] * 3, {}), x_T=noise,
                                      guidance_scale=guidance, unconditional_conditioning=(ne.repeat(3, 1, 1), [w.negative_prompt] * 3, {}),
                                      generator=torch.Generator().manual_seed(5))
    assert torch.equal(out, ref)
    other = w(noise, None, prompt_embeds=(pe, ne), guidance_scale=guidance, out_image_count=3, generator=torch.Generator().manual_seed(6))
    assert bool(torch.isfinite(other).all()) and not torch.equal(other, out)


def test_wrapper_img2img_lcm(dev):
    """img2img with use_lcm, 4 steps, strength 0.5: U-Net calls at 499 and 259 (g = 1.5: batch 2 x 2); 4 PIL images."""
    pe, ne = _embs(dev)
    w = _wrapper(dev, "img2img")
    img = Image.fromarray(np.random.default_rng(5).integers(0, 256, (128, 128, 3), dtype=np.uint8))
    calls = _spy_calls(w.ldm)
    try:
        out = w(img, None, prompt_embeds=(pe, ne), guidance_scale=1.5, out_image_count=2, ref_img_strength=0.5,
                generator=torch.Generator().manual_seed(9))
    finally:
        del w.ldm.apply_model
    assert calls == [(499, 4), (259, 4)]
    assert len(out) == 2 and out[0].size == (128, 128)


def test_wrapper_fuse_unfuse_restores_ddim_output(dev):
    """A DDIM wrapper that fused the LoRA, ran on the fused weights (its packs rebuilt) and unfused it gives bitwise the output of a
    wrapper that never fused; the fused run differs."""
    from adaface_dev_amd import rng
    pe, ne = _embs(dev)
    noise = rng.synth_input("lcm.noise", (2, 4, 16, 16), seed=83).to(dev)
    plain = _wrapper(dev, use_lcm=False, steps=5)
    ref = plain(noise, None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=2)
    w = _wrapper(dev, use_lcm=False, steps=5)
    w(noise, None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=2)
    w.fuse_lcm_lora(_lora(w.ldm), 1.0)
    fused = w(noise, None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=2)
    w.unfuse_lcm_lora()
    out = w(noise, None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=2)
    assert torch.equal(out, ref) and not torch.equal(fused, ref)
