"""DPM-Solver++ on a real MI355X (`pytest -m gpu`): the fused guidance + DPM-Solver++ kernel af_cfg_dpmpp_step against the fp64
restatement (dpmpp_restatement.py), DPMSolverSampler on a Gaussian data model (order of convergence through the kernel), the SD-1.5 U-Net
trajectory against the CPU oracle, and AdaFaceWrapper(default_scheduler_name="dpm++") at reduced width."""
import time

import numpy as np
import pytest
import torch
from PIL import Image

import dpmpp_restatement as R
from conftest import rel_l2
from test_dpmpp_host import MU, SD, check_second_order
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
    return R.sd15_alphas_cumprod()


# ---------------------------------------------------------------------------------------------------------------- kernel
def _step_case(ac, kind):
    """(guidance, alpha_s, sigma_s, c_base, c0, c1) of one step of the 20-step schedule: order 1 (t = 999), order 2 (t = 949, block
    from 999), the final step (t = 50 -> x0)."""
    co = R.coefficients(ac, R.timesteps(20), R.orders(20))
    k = {"order1": 0, "order2": 1, "final": 19}[kind]
    return (4.0,) + tuple(co[k][:5])


def _kernel_ref(ec, eu, x, xb, xp, has_uncond, g, a_s, s_s, c_base, c0, c1):
    """fp64 reference and the magnitude of the terms each output is summed from (relative errors are taken against it)."""
    ec, eu, x, xb, xp = (t.double() for t in (ec, eu, x, xb, xp))
    if has_uncond:
        e, e_mag = eu + g * (ec - eu), eu.abs() + abs(g) * (ec.abs() + eu.abs())
    else:
        e, e_mag = ec, ec.abs()
    x0 = (x - s_s * e) / a_s
    x0_mag = (x.abs() + s_s * e_mag) / a_s
    out = c_base * xb + c0 * x0 + c1 * xp
    out_mag = abs(c_base) * xb.abs() + abs(c0) * x0_mag + abs(c1) * xp.abs()
    return out, x0, out_mag, x0_mag


# fp32 evaluation of a handful of operations: bound 1e-6 of the term magnitude (8 ulp); measured on MI355X at most 2.44e-7
KERNEL_TOL = 1e-6
# two fp32 evaluations of the same step in different forms (x0 form here, epsilon form in af_cfg_ddim_step), each error taken against
# the x0 form's term magnitude: bound 4e-6; measured on MI355X at most 9.7e-7 (x_out) and 2.3e-7 (x0)
DDIM_FORM_TOL = 4e-6


@pytest.mark.parametrize("n", [4 * 4 * 64 * 64, 4 * 4 * 96 * 64, 1001])
@pytest.mark.parametrize("has_uncond", [True, False])
@pytest.mark.parametrize("kind", ["order1", "order2", "final"])
def test_kernel_vs_fp64(dev, ac, n, has_uncond, kind):
    """af_cfg_dpmpp_step (16-byte path for n % 4 == 0, scalar path for n = 1001) against the fp64 restatement, error relative to the
    magnitude of the summed terms.  Bound 1e-6; measured on MI355X: 1.1e-7 .. 2.4e-7 over these cases (order 2 the largest)."""
    from adaface_dev_amd import ops
    g = torch.Generator().manual_seed(n + 7 * has_uncond)
    ec, eu, x, xb, xp = (torch.randn(n, generator=g) for _ in range(5))
    eps2 = torch.cat([ec, eu]) if has_uncond else ec.clone()
    gd, a_s, s_s, c_base, c0, c1 = _step_case(ac, kind)
    xb_d = xb.to(dev) if kind == "order2" else x.to(dev)
    xp_d = xp.to(dev) if c1 != 0.0 else None
    x_out, x0_out = ops.cfg_dpmpp_step(eps2.to(dev), x.to(dev), xb_d, xp_d, gd, a_s, s_s, c_base, c0, c1, has_uncond)
    assert torch.isfinite(x_out).all() and torch.isfinite(x0_out).all()
    ref, ref_x0, mag, mag_x0 = _kernel_ref(ec, eu, x, xb_d.cpu(), xp if xp_d is not None else torch.zeros(n), has_uncond, gd, a_s, s_s,
                                           c_base, c0, c1)
    err = float(((x_out.cpu().double() - ref).abs() / mag.clamp_min(1e-30)).max())
    err0 = float(((x0_out.cpu().double() - ref_x0).abs() / mag_x0.clamp_min(1e-30)).max())
    print(f"cfg_dpmpp_step n={n} uncond={has_uncond} {kind}: term-relative error x_out {err:.2e}, x0 {err0:.2e}")
    assert err < KERNEL_TOL and err0 < KERNEL_TOL
    if kind == "final":
        assert torch.equal(x_out, x0_out)


@pytest.mark.parametrize("n", [4 * 4 * 64 * 64, 1001])
def test_kernel_does_not_read_x0_prev_when_c1_is_zero(dev, ac, n):
    """A NaN-filled x0_prev handed to the C ABI with c1 = 0 leaves the output finite and equal to the NULL-pointer launch."""
    from adaface_dev_amd import _lib, ops
    g = torch.Generator().manual_seed(n)
    eps2, x = torch.randn(2 * n, generator=g).to(dev), torch.randn(n, generator=g).to(dev)
    gd, a_s, s_s, c_base, c0, c1 = _step_case(ac, "order1")
    assert c1 == 0.0
    ref_out, ref_x0 = ops.cfg_dpmpp_step(eps2, x, x, None, gd, a_s, s_s, c_base, c0, 0.0, True)
    nan_prev = torch.full((n,), float("nan"), device=dev)
    x_out, x0_out = torch.empty_like(x), torch.empty_like(x)
    rc = _lib.lib().af_cfg_dpmpp_step(eps2.data_ptr(), x.data_ptr(), x.data_ptr(), nan_prev.data_ptr(), x_out.data_ptr(),
                                      x0_out.data_ptr(), n, 1, gd, a_s, s_s, c_base, c0, 0.0, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.isfinite(x_out).all() and torch.equal(x_out, ref_out) and torch.equal(x0_out, ref_x0)


@pytest.mark.parametrize("n", [4 * 4 * 64 * 64, 1001])
@pytest.mark.parametrize("t_s,t_t", [(999, 949), (500, 450), (100, 50)])
def test_order1_step_matches_ddim_kernel(dev, ac, n, t_s, t_t):
    """DPM-Solver-1 is DDIM: an order-1 step equals af_cfg_ddim_step with a_t = abar_s, a_prev = abar_t within fp32 rounding
    (DDIM_FORM_TOL; measured on MI355X: x_out 3.1e-7 .. 9.7e-7, x0 0 .. 2.3e-7)."""
    from adaface_dev_amd import ops
    from adaface_dev_amd.ldm.models.diffusion.dpm_solver import dpmpp_step_coefficients
    g = torch.Generator().manual_seed(n + t_s)
    eps2, x = torch.randn(2 * n, generator=g).to(dev), torch.randn(n, generator=g).to(dev)
    a_s, s_s, c_base, c0, c1, _ = dpmpp_step_coefficients(ac.numpy(), [t_s, t_t, 0], [1, 1, 1])[0]
    x_out, x0_out = ops.cfg_dpmpp_step(eps2, x, x, None, 5.0, a_s, s_s, c_base, c0, c1, True)
    x_dd, x0_dd = ops.cfg_ddim_step(eps2, x, 5.0, float(ac[t_s]), float(ac[t_t]), True)
    _, _, mag, mag_x0 = _kernel_ref(eps2[:n].cpu(), eps2[n:].cpu(), x.cpu(), x.cpu(), torch.zeros(n), True, 5.0, a_s, s_s, c_base, c0, 0.0)
    err = float(((x_out - x_dd).abs().cpu().double() / mag).max())
    err0 = float(((x0_out - x0_dd).abs().cpu().double() / mag_x0).max())
    print(f"order 1 vs ddim kernel n={n} {t_s}->{t_t}: x_out {err:.2e}, x0 {err0:.2e}")
    assert err < DDIM_FORM_TOL and err0 < DDIM_FORM_TOL


def test_kernel_refuses_bad_arguments(dev):
    from adaface_dev_amd import _lib
    L = _lib.lib()
    n = 64
    b = [torch.zeros(2 * n, device=dev) for _ in range(6)]
    p = [t.data_ptr() for t in b]

    def call(ptrs=p, nn=n, g=4.0, a_s=0.5, s_s=0.8, c_base=0.6, c0=0.5, c1=0.2):
        return L.af_cfg_dpmpp_step(*ptrs, nn, 1, g, a_s, s_s, c_base, c0, c1, None)

    assert call() == 0
    torch.cuda.synchronize()
    for i in (0, 1, 2, 4, 5):
        assert call(ptrs=[None if j == i else q for j, q in enumerate(p)]) == _lib.AF_E_BADARG, i
    assert call(ptrs=[None if j == 3 else q for j, q in enumerate(p)]) == _lib.AF_E_BADARG        # c1 != 0 needs x0_prev
    assert call(ptrs=[None if j == 3 else q for j, q in enumerate(p)], c1=0.0) == 0
    torch.cuda.synchronize()
    for kw in (dict(nn=0), dict(nn=-4), dict(a_s=0.0), dict(a_s=-0.5), dict(a_s=1.5), dict(s_s=1.0), dict(s_s=-0.1),
               dict(c0=float("nan")), dict(c_base=float("inf")), dict(c1=float("-inf")), dict(g=float("nan"))):
        assert call(**kw) == _lib.AF_E_BADARG, kw
    assert b"af_cfg_dpmpp_step" in L.af_last_error()


# ---------------------------------------------------------------------------------------------------------------- Gaussian model
class _GaussianModel:
    """Stand-in for LatentDiffusion whose apply_model returns the exact epsilon of x0 ~ N(MU, SD^2)."""

    def __init__(self, ac, dev):
        self.num_timesteps = 1000
        self.alphas_cumprod = ac.to(dev)
        self.betas = torch.zeros(1000, device=dev)
        self._ac = ac
        self.calls = 0

    def apply_model(self, x, t, c):
        self.calls += 1
        a, s = R.alpha_sigma(self._ac, int(t[0]))
        return R.gaussian_eps(x, a, s, MU, SD)


def _gaussian_sampler_errors(dev, ac):
    from adaface_dev_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    x_T = torch.linspace(-3, 3, 64, dtype=torch.float64)
    mid, last = [], []
    for N in (10, 20, 40):
        m = _GaussianModel(ac, dev)
        lat, inter = DPMSolverSampler(m).sample(N, 1, (4, 4, 4), conditioning=None, x_T=x_T.float().reshape(1, 4, 4, 4).to(dev),
                                                log_every_t=1)
        xs = inter["x_inter"]
        assert m.calls == N and len(xs) == N + 1 and torch.equal(xs[-1], lat)
        ts = R.timesteps(N)
        aT, sT = R.alpha_sigma(ac, ts[0])
        for k, out in ((N // 2, mid), (N - 1, last)):
            ref = R.gaussian_flow(x_T, aT, sT, *R.alpha_sigma(ac, ts[k]), MU, SD)
            out.append(float((xs[k].reshape(-1).double().cpu() - ref).abs().max()))
    return mid, last


def test_sampler_gaussian_convergence(dev, ac, monkeypatch):
    """DPMSolverSampler.sample through af_cfg_dpmpp_step (no guidance), the stand-in model returning the exact epsilon; the same
    check as test_dpmpp_host.test_gaussian_convergence_second_order.  Measured on MI355X (fp32), errors at t = 500 for N = 10, 20, 40:
    5.34e-3, 7.53e-4, 1.91e-4 (ratios 7.09, 3.93; bound >= 3.5), within 1e-3 relative of the fp64 iteration.  Negative control: every
    order forced to 1 gives 8.07e-3, 4.05e-3, 2.03e-3 (ratios 1.99, 2.00) and fails the check."""
    from adaface_dev_amd.ldm.models.diffusion import dpm_solver
    mid, last = _gaussian_sampler_errors(dev, ac)
    print(f"sampler order 2: errors at t = 500 {mid}, before the final step {last}")
    check_second_order(mid, last)
    monkeypatch.setattr(dpm_solver, "dpmpp_orders", lambda n: [1] * n)
    mid1, last1 = _gaussian_sampler_errors(dev, ac)
    print(f"sampler all order 1: errors at t = 500 {mid1}, before the final step {last1}")
    with pytest.raises(AssertionError):
        check_second_order(mid1, last1)


# ---------------------------------------------------------------------------------------------------------------- SD-1.5 vs oracle
class _Full:
    pass


@pytest.fixture(scope="module")
def full(dev):
    """LatentDiffusion(SD15_UNET_CONFIG) with synthetic weights drawn on the device (seed 0), one image, contexts at seed 52."""
    from adaface_dev_amd import SD15_UNET_CONFIG, rng
    from adaface_dev_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    with rng.skip_default_init():
        ldm = LatentDiffusion(SD15_UNET_CONFIG)
    ldm = ldm.to(dev).eval()
    unet = ldm.model.diffusion_model
    rng.load_synth_weights(unet, seed=0, on_device=True)
    unet.prepare()
    for p in unet.parameters():
        p.requires_grad_(False)
    f = _Full()
    f.cfg, f.ldm = SD15_UNET_CONFIG, ldm
    f.x = rng.synth_input("dpm.x", (1, 4, 64, 64), seed=52)
    f.c = rng.synth_input("dpm.ctx", (1, 77, 768), seed=52)
    f.u = rng.synth_input("dpm.uctx", (1, 77, 768), seed=52)
    f.sd = {k: v.detach().float().cpu() for k, v in unet.state_dict().items()}
    f.ac = ldm.alphas_cumprod.detach().double().cpu()
    yield f
    del f.sd
    torch.cuda.synchronize()


# 2x the worst per-step value measured on MI355X (docstring of test_trajectory_vs_oracle)
TRAJ_TOL = {"first4": {"pred_x0": 5.4e-3, "update": 5.5e-3, "teacher_eps": 8.0e-3},
            "img2img_tail": {"pred_x0": 3.0e-3, "update": 7.2e-3, "teacher_eps": 7.6e-3}}


@pytest.mark.parametrize("segment", ["first4", "img2img_tail"])
def test_trajectory_vs_oracle(dev, full, segment):
    """DPMSolverSampler on the SD-1.5 U-Net (synthetic weights, one image, cond + uncond, guidance 4) against oracle.unet_forward
    driven by the fp64 restatement.  first4: the first 4 steps of sample(20) (t = 999, 949, 899, 849; orders 1, 2, 1, 2) from
    dpm.x.  img2img_tail: sample_img2img(20, 0.15) -- t = 150, 100, 50; orders 1, 2, 1 -- from q_sample(x0, t = 150).
    Per step: pred_x0, the accumulated update x_k - x_T, and the teacher-forced guided epsilon (the GPU U-Net on the oracle's own x_k).
    Worst step measured on MI355X (the bounds TRAJ_TOL are 2x):
        first4        pred_x0 2.72e-3, x_k - x_T 2.73e-3, teacher-forced eps 4.02e-3 (all at t = 999, falling over the 4 steps)
        img2img_tail  pred_x0 1.49e-3, x_k - x_T 3.58e-3, teacher-forced eps 3.82e-3 (all at t = 150)
    These are the DDIM trajectory test's levels (test_hip_bench_shape.py): the error is the U-Net's, and the order-2 steps add none.
    The oracle costs about 19 s + 13 s of CPU."""
    from adaface_dev_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from oracle import diffusion_oracle as D
    from oracle import unet_oracle as O
    ldm = full.ldm
    s = DPMSolverSampler(ldm)
    c = (full.c.to(dev), [""], {})
    u = (full.u.to(dev), [""], {})
    calls = []
    orig = ldm.apply_model

    def spy(x, t, cc, **kw):
        calls.append(int(t[0]))
        return orig(x, t, cc, **kw)

    ldm.apply_model = spy
    try:
        if segment == "first4":
            x_T = full.x.to(dev)
            ts, ords = R.timesteps(20), R.orders(20)
            lat, inter = s.sample(20, 1, (4, 64, 64), conditioning=c, x_T=x_T, guidance_scale=4.0, unconditional_conditioning=u,
                                  log_every_t=1)
            n_check = 4
        else:
            n, t_first, ts, ords = R.img2img(20, 0.15)
            assert s.img2img_steps(20, 0.15) == (n, t_first) == (3, 150) and ts == [150, 100, 50] and ords == [1, 2, 1]
            x0 = rng_input("dpm.i2i.x0")
            noise = rng_input("dpm.i2i.noise")
            tt = torch.full((1,), t_first, dtype=torch.int64)
            x_T = ldm.q_sample(x0.to(dev), tt.to(dev), noise.to(dev))
            tabs = D.register_schedule(D.make_beta_schedule_linear())
            assert rel_l2(x_T.cpu().numpy(), D.q_sample(tabs, x0, tt, noise).numpy()) < 1e-6
            lat, inter = s.sample_img2img(20, 0.15, 1, x_T, c, guidance_scale=4.0, unconditional_conditioning=u, log_every_t=1)
            n_check = 3
    finally:
        del ldm.apply_model
    assert calls == ts and len(inter["x_inter"]) == len(ts) + 1
    gx, gx0 = inter["x_inter"], inter["pred_x0"][1:]

    t0 = time.perf_counter()
    xT = x_T.cpu()
    scales = R.guide_scales(len(ts), 4.0)
    errs = []

    def eps_fn(x, t, i):
        with torch.no_grad():
            e2 = O.unet_forward(full.sd, full.cfg, torch.cat([x, x]).float(), torch.tensor([t, t]), torch.cat([full.c, full.u]), {})
        e_o = e2[1:].double() + scales[i] * (e2[:1].double() - e2[1:].double())
        # teacher forcing: the GPU U-Net on the oracle's x_k
        with torch.no_grad():
            xd = x.float().to(dev)
            e2_g = ldm.apply_model(torch.cat([xd, xd]), torch.full((2,), t, dtype=torch.int64, device=dev),
                                   (torch.cat([c[0], u[0]]), ["", ""], {})).cpu().double()
        e_tf = e2_g[1:] + scales[i] * (e2_g[:1] - e2_g[1:])
        errs.append({"teacher_eps": rel_l2(e_tf.numpy(), e_o.numpy())})
        return e_o

    xo, x0o = R.run(full.ac, ts, ords, xT, eps_fn, n_steps=n_check)
    tol = TRAJ_TOL[segment]
    worst = dict.fromkeys(tol, 0.0)
    for i in range(n_check):
        errs[i]["pred_x0"] = rel_l2(gx0[i].cpu().numpy(), x0o[i].numpy())
        errs[i]["update"] = rel_l2((gx[i + 1].cpu() - xT).numpy(), (xo[i + 1] - xT).numpy())
        e = errs[i]
        print(f"{segment} step {i} (t = {ts[i]}, order {ords[i]}): pred_x0 {e['pred_x0']:.3e}  x_k - x_T {e['update']:.3e}  "
              f"teacher-forced eps {e['teacher_eps']:.3e}")
        for k, v in e.items():
            worst[k] = max(worst[k], v)
    print(f"{segment}: oracle {2 * n_check} sample-forwards in {time.perf_counter() - t0:.1f} s; worst {worst}")
    for k, v in worst.items():
        assert v < tol[k], (k, v)


def rng_input(name):
    from adaface_dev_amd import rng
    return rng.synth_input(name, (1, 4, 64, 64), seed=53)


# ---------------------------------------------------------------------------------------------------------------- wrapper
def _unet_cfg():
    from adaface_dev_amd import TINY_UNET_CONFIG
    return dict(TINY_UNET_CONFIG, model_channels=64, context_dim=128)


def _wrapper(dev, pipeline_name, scheduler, steps):
    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper
    from adaface_dev_amd.adaface.arc2face_models import clip_text_config
    cc = clip_text_config(hidden_size=128, num_attention_heads=2, num_hidden_layers=3, intermediate_size=512)
    w = AdaFaceWrapper(pipeline_name=pipeline_name, clip_config=cc, unet_config=_unet_cfg(), device=dev, num_inference_steps=steps,
                       default_scheduler_name=scheduler)
    rng.load_synth_weights(w.ldm.model.diffusion_model, seed=63)
    if pipeline_name == "img2img":
        ae = w.ldm.instantiate_first_stage(dict(VAE_SMALL, double_z=True))
        with torch.no_grad():
            for n, p in ae.named_parameters():
                p.copy_(rng.synth_tensor(n, p.shape, seed=92))
        w.vae = ae
    return w.to(dev)


def _spy_calls(ldm):
    calls = []
    orig = ldm.apply_model

    def spy(x, t, c, **kw):
        calls.append(int(t[0]))
        return orig(x, t, c, **kw)

    ldm.apply_model = spy
    return calls


def _embs(dev):
    from adaface_dev_amd import rng
    return rng.synth_input("dpm.pe", (1, 77, 128), seed=80).to(dev), rng.synth_input("dpm.ne", (1, 77, 128), seed=81).to(dev)


def test_wrapper_text2img_dpmpp(dev):
    """text2img with "dpm++" and 20 steps: bitwise DPMSolverSampler.sample driven by hand, 20 U-Net calls on R.timesteps(20);
    a "ddim" wrapper on the same weights stays bitwise DDIMSampler.sample."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.models.diffusion.ddim import DDIMSampler
    from adaface_dev_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    pe, ne = _embs(dev)
    noise = rng.synth_input("dpm.noise", (3, 4, 16, 16), seed=82).to(dev)
    w = _wrapper(dev, "text2img", "dpm++", 20)
    calls = _spy_calls(w.ldm)
    try:
        out = w(noise, None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=3)
    finally:
        del w.ldm.apply_model
    assert calls == R.timesteps(20)
    assert out.shape == (3, 4, 16, 16) and bool(torch.isfinite(out).all())
    cond = (pe.repeat(3, 1, 1), [""] * 3, {})
    uncond = (ne.repeat(3, 1, 1), [w.negative_prompt] * 3, {})
    ref, _ = DPMSolverSampler(w.ldm).sample(20, 3, (4, 16, 16), conditioning=cond, x_T=noise, guidance_scale=4.0,
                                            unconditional_conditioning=uncond)
    assert torch.equal(out, ref)

    d = _wrapper(dev, "text2img", "ddim", 5)
    out_d = d(noise, None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=3)
    ref_d, _ = DDIMSampler(d.ldm).sample(5, 3, (4, 16, 16), conditioning=cond, x_T=noise, verbose=False, guidance_scale=4.0,
                                         unconditional_conditioning=(ne.repeat(3, 1, 1), [d.negative_prompt] * 3, {}))
    assert torch.equal(out_d, ref_d)
    assert not torch.equal(out_d, out)


def _pil(seed):
    return Image.fromarray(np.random.default_rng(seed).integers(0, 256, (128, 128, 3), dtype=np.uint8))


def test_wrapper_img2img_dpmpp(dev):
    """img2img with "dpm++" over 20 steps: strength 1.0 decodes bitwise what a text2img run (DPMSolverSampler.sample) from the same
    x_t decodes; strength 0.15 makes 3 U-Net calls at t = 150, 100, 50."""
    from adaface_dev_amd.adaface.adaface_wrapper import img2img_images_u8
    from adaface_dev_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    pe, ne = _embs(dev)
    w = _wrapper(dev, "img2img", "dpm++", 20)
    img = _pil(5)
    calls = _spy_calls(w.ldm)
    try:
        out = w(img, None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=2, ref_img_strength=1.0,
                generator=torch.Generator().manual_seed(9))
        n_full = len(calls)
        low = w(img, None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=2, ref_img_strength=0.15,
                generator=torch.Generator().manual_seed(9))
    finally:
        del w.ldm.apply_model
    assert n_full == 20 and calls[20:] == [150, 100, 50]
    s = DPMSolverSampler(w.ldm)
    assert s.img2img_steps(20, 1.0) == (20, 999)
    x_t = w.ldm.img2img_latents(img2img_images_u8(img, 2).to(dev), 2, 999, generator=torch.Generator().manual_seed(9),
                                first_stage_model=w.vae)
    lat, _ = s.sample(20, 2, (4, 16, 16), conditioning=(pe.repeat(2, 1, 1), [""] * 2, {}), x_T=x_t, guidance_scale=4.0,
                      unconditional_conditioning=(ne.repeat(2, 1, 1), [w.negative_prompt] * 2, {}))
    dec = w.vae.decode(lat / 0.18215)
    man = ((dec.float() / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
    assert [np.asarray(im).tobytes() for im in out] == [m.tobytes() for m in man]
    assert len(low) == 2 and [np.asarray(im).tobytes() for im in low] != [m.tobytes() for m in man]
