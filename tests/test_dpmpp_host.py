"""DPM-Solver++ host logic, CPU only: the schedule, the solver orders, img2img truncation and the fp64 step coefficients of
adaface_dev_amd.ldm.models.diffusion.dpm_solver against literals and against the independent restatement in dpmpp_restatement.py
(INTEGRATION.md "DPM-Solver++ scheduler"), the order of convergence on a Gaussian data model, and the wrapper's scheduler names."""
import math
import types

import numpy as np
import pytest
import torch

import dpmpp_restatement as R
from adaface_dev_amd import TINY_UNET_CONFIG
from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper
from adaface_dev_amd.adaface.arc2face_models import clip_text_config
from adaface_dev_amd.ldm.models.diffusion.dpm_solver import (DPMSolverSampler, dpmpp_orders, dpmpp_step_coefficients,
                                                             dpmpp_timesteps)

TIMESTEPS = {
    10: [999, 899, 799, 699, 599, 500, 400, 300, 200, 100],
    20: [999, 949, 899, 849, 799, 749, 699, 649, 599, 549, 500, 450, 400, 350, 300, 250, 200, 150, 100, 50],
    25: [999, 959, 919, 879, 839, 799, 759, 719, 679, 639, 599, 559, 519, 480, 440, 400, 360, 320, 280, 240, 200, 160, 120, 80, 40],
    50: [999, 979, 959, 939, 919, 899, 879, 859, 839, 819, 799, 779, 759, 739, 719, 699, 679, 659, 639, 619, 599, 579, 559, 539, 519,
         500, 480, 460, 440, 420, 400, 380, 360, 340, 320, 300, 280, 260, 240, 220, 200, 180, 160, 140, 120, 100, 80, 60, 40, 20],
}
ORDERS = {1: [1], 2: [1, 1], 3: [1, 2, 1], 4: [1, 2, 1, 1], 5: [1, 2, 1, 2, 1], 6: [1, 2, 1, 2, 1, 1],
          20: [1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 1]}


def _ac():
    """The package's own SD-1.5 table (LatentDiffusion.register_schedule, stored fp32), in fp64."""
    from adaface_dev_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    ac = LatentDiffusion(dict(TINY_UNET_CONFIG)).alphas_cumprod.double()
    assert float((ac - R.sd15_alphas_cumprod()).abs().max()) < 1e-7         # the SD-1.5 schedule, rounded to fp32
    return ac


@pytest.fixture(scope="module")
def ac():
    return _ac()


def _sampler():
    return DPMSolverSampler(types.SimpleNamespace(num_timesteps=1000))


@pytest.mark.parametrize("S", sorted(TIMESTEPS))
def test_timesteps_literal(S):
    ts = dpmpp_timesteps(S)
    assert ts.dtype == np.int64 and ts.tolist() == TIMESTEPS[S]
    assert R.timesteps(S) == TIMESTEPS[S]


@pytest.mark.parametrize("n", sorted(ORDERS))
def test_orders_literal(n):
    assert dpmpp_orders(n) == ORDERS[n] == R.orders(n)


def test_orders_rules():
    for n in range(1, 60):
        o = dpmpp_orders(n)
        assert len(o) == n and o[-1] == 1 and o[0] == 1
        assert all(o[k - 1] == 1 for k in range(1, n) if o[k] == 2)          # an order-2 step follows an order-1 step


def test_img2img_known_answers():
    s = _sampler()
    assert s.img2img_steps(50, 0.8) == (40, 799)
    assert s.img2img_steps(50, 0.58) == (28, 559)             # int(28.999...) = 28
    assert s.img2img_steps(50, 0.9) == (45, 899)
    assert s.img2img_steps(50, 1.0) == (50, 999)
    assert s.img2img_steps(50, 0.02) == (1, 20)
    assert s.img2img_steps(20, 0.15) == (3, 150)
    for st in (0.8, 0.58, 0.9, 1.0, 0.02):
        assert s.img2img_steps(50, st) == R.img2img(50, st)[:2]


@pytest.mark.parametrize("strength", [0, 0.019, -0.1, 1.2])
def test_img2img_refuses_bad_strength(strength):
    with pytest.raises(ValueError):
        _sampler().img2img_steps(50, strength)


@pytest.mark.parametrize("n", [1, 2, 5, 20])
def test_last_step_is_x0(ac, n):
    co = dpmpp_step_coefficients(ac.numpy(), dpmpp_timesteps(n), dpmpp_orders(n))
    assert co[-1][2:5] == (0.0, 1.0, 0.0) and co[-1][5] is False


def test_coefficients_refuse_bad_orders(ac):
    ts = dpmpp_timesteps(4)
    for bad in ([2, 1, 1, 1], [1, 2, 2, 1], [1, 2, 1, 2], [1, 1, 1]):
        with pytest.raises(ValueError):
            dpmpp_step_coefficients(ac.numpy(), ts, bad)


def _close(a, b, tol=1e-12):
    return all(abs(x - y) <= tol * max(1.0, abs(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("case", ["S10", "S20", "S25", "S50", "i2i50_0.58", "i2i20_0.15", "i2i50_0.02", "S20_all1"])
def test_coefficients_match_restatement(ac, case):
    if case.startswith("S"):
        S = int(case[1:].split("_")[0])
        ts = R.timesteps(S)
        ords = [1] * S if case.endswith("all1") else R.orders(S)
    else:
        S, st = case[3:].split("_")
        _, _, ts, ords = R.img2img(int(S), float(st))
    mine = dpmpp_step_coefficients(ac.numpy(), ts, ords)
    ref = R.coefficients(ac, ts, ords)
    assert len(mine) == len(ref)
    for k, (m, r) in enumerate(zip(mine, ref)):
        assert m[5] == r[5], (k, m, r)
        assert _close(m[:5], r[:5]), (k, m, r)


def test_order1_step_is_ddim(ac):
    """DPM-Solver-1 is DDIM: an order-1 step between two timesteps is the eta = 0 DDIM update a_t = abar_s, a_prev = abar_t."""
    g = torch.Generator().manual_seed(0)
    x, x0 = torch.randn(1000, generator=g, dtype=torch.float64), torch.randn(1000, generator=g, dtype=torch.float64)
    for s, t in ((999, 949), (500, 450), (100, 50), (959, 919), (40, 20), (999, 500)):
        a_s, s_s, c_base, c0, c1, blk = dpmpp_step_coefficients(ac.numpy(), [s, t, 0], [1, 1, 1])[0]
        assert c1 == 0.0 and not blk
        a_t, a_prev = float(ac[s]), float(ac[t])
        e = (x - math.sqrt(a_t) * x0) / math.sqrt(1 - a_t)
        ddim = math.sqrt(a_prev) * x0 + math.sqrt(1 - a_prev) * e
        dpm = c_base * x + c0 * x0
        assert float((dpm - ddim).abs().max()) < 1e-12, (s, t)
        assert (a_s, s_s) == (math.sqrt(a_t), math.sqrt(1 - a_t))


# ---------------------------------------------------------------------------------------------------------------- convergence
MU, SD = 0.5, 0.3


def gaussian_errors(ac, iterate, orders_fn, Ns=(10, 20, 40)):
    """Error of the sampler against the probability-flow solution on x0 ~ N(MU, SD^2): at x_{N/2} (timestep 500 for every even N,
    a fixed point of the ODE) and at x_{N-1}, the sample before the final x0 step.  iterate(ts, ords, x_T, eps_fn) -> [x_0 .. x_N]."""
    x_T = torch.linspace(-3, 3, 61, dtype=torch.float64)
    mid, last = [], []
    for N in Ns:
        ts, ords = R.timesteps(N), orders_fn(N)
        eps = lambda x, t: R.gaussian_eps(x, *R.alpha_sigma(ac, t), MU, SD)
        xs = iterate(ts, ords, x_T, eps)
        aT, sT = R.alpha_sigma(ac, ts[0])
        for k, out in ((N // 2, mid), (N - 1, last)):
            ref = R.gaussian_flow(x_T, aT, sT, *R.alpha_sigma(ac, ts[k]), MU, SD)
            out.append(float((xs[k].double().cpu() - ref).abs().max()))
    return mid, last


def _iterate_coefficients(ac):
    def it(ts, ords, x_T, eps):
        co = dpmpp_step_coefficients(ac.numpy(), ts, ords)
        xs, blk = [x_T], None
        for t, (a_s, s_s, c_base, c0, c1, uses_blk) in zip(ts, co):
            x = xs[-1]
            x0 = (x - s_s * eps(x, t)) / a_s
            xb, x0p = blk if uses_blk else (x, torch.zeros_like(x))
            xs.append(c_base * xb + c0 * x0 + c1 * x0p)
            if not uses_blk:
                blk = (x, x0)
        return xs
    return it


# at timestep 500 the error ratio N -> 2N of a second-order solver is about 4 (measured in fp64: 7.09 at 10 -> 20, 3.93 at 20 -> 40);
# with every step order 1 it is 2 (1.99, 2.00).  The bound sits between them.
MIN_RATIO = 3.5


def check_second_order(mid, last):
    ratios = [mid[i] / mid[i + 1] for i in range(len(mid) - 1)]
    assert all(r >= MIN_RATIO for r in ratios), (mid, ratios)
    assert last[0] > last[1] > last[2], last            # the error before the final step falls too (more slowly: see docstring)


def test_gaussian_convergence_second_order(ac):
    """x0 ~ N(0.5, 0.3^2) element-wise, 61 values of x_T in [-3, 3], N = 10, 20, 40, the package coefficients iterated in fp64.
    Measured max errors at x_{N/2} (t = 500): 5.34e-3, 7.53e-4, 1.91e-4 (ratios 7.09, 3.93; bound >= 3.5).  At x_{N-1}: 4.39e-2,
    2.93e-2, 1.74e-2 (ratios 1.50, 1.69): the linspace schedule does not refine near t = 0 in log-SNR (lambda(2d) - lambda(d) is
    about log(2) / 2 for every spacing d), so the sample just before the final step converges below second order; it is only checked
    to fall.  Negative control: with every order forced to 1 the t = 500 errors are 8.07e-3, 4.05e-3, 2.03e-3 (ratios 1.99, 2.00) and
    the order check fails."""
    it = _iterate_coefficients(ac)
    mid, last = gaussian_errors(ac, it, dpmpp_orders)
    print(f"dpm++ order 2: errors at t = 500 {mid}, before the final step {last}")
    check_second_order(mid, last)
    # the restatement's own loop agrees with the coefficients
    mid_r, last_r = gaussian_errors(ac, lambda ts, o, x, e: R.run(ac, ts, o, x, lambda xx, t, i: e(xx, t))[0], R.orders)
    assert np.allclose(mid, mid_r, rtol=1e-9, atol=1e-15) and np.allclose(last, last_r, rtol=1e-9, atol=1e-15)
    # negative control
    mid1, last1 = gaussian_errors(ac, it, lambda n: [1] * n)
    print(f"all order 1: errors at t = 500 {mid1}, before the final step {last1}")
    with pytest.raises(AssertionError):
        check_second_order(mid1, last1)
    assert all(m < m1 for m, m1 in zip(mid, mid1))


# ---------------------------------------------------------------------------------------------------------------- wrapper
def _wrapper(pipeline_name="text2img", **kw):
    cc = clip_text_config(hidden_size=64, num_attention_heads=1, num_hidden_layers=1, intermediate_size=128)
    return AdaFaceWrapper(pipeline_name=pipeline_name, clip_config=cc, unet_config=dict(TINY_UNET_CONFIG), device="cpu", **kw)


@pytest.mark.parametrize("pipeline_name", ["text2img", "img2img"])
def test_wrapper_scheduler_names(pipeline_name):
    from adaface_dev_amd.ldm.models.diffusion.ddim import DDIMSampler
    w = _wrapper(pipeline_name, default_scheduler_name="dpm++")
    assert w.default_scheduler_name == "dpm++" and isinstance(w._sampler(), DPMSolverSampler)
    d = _wrapper(pipeline_name)
    assert d.default_scheduler_name == "ddim" and isinstance(d._sampler(), DDIMSampler)
    for bad in ("pndm", "dpm", "DDIM", "lcm"):
        with pytest.raises(NotImplementedError):
            _wrapper(pipeline_name, default_scheduler_name=bad)
    for name in ("ddim", "dpm++"):
        with pytest.raises(NotImplementedError):
            _wrapper(pipeline_name, default_scheduler_name=name, use_lcm=True)


def test_wrapper_dpmpp_img2img_refuses_bad_strength_before_gpu_work():
    from PIL import Image
    from test_vae_oracle import VAE_SMALL
    w = _wrapper("img2img", default_scheduler_name="dpm++", num_inference_steps=20)
    w.ldm.instantiate_first_stage(dict(VAE_SMALL, double_z=True))
    w.vae = w.ldm.first_stage_model
    pe = torch.zeros(1, 77, 64)
    img = Image.fromarray(np.zeros((64, 64, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="strength"):
        w(img, None, prompt_embeds=(pe, pe), out_image_count=1, ref_img_strength=0.04)     # int(20 * 0.04) = 0
