"""DPM-Solver++ sampling (Lu et al., 2022): the reference wrapper's ``"dpm++"`` scheduler, restated from diffusers'
``DPMSolverSinglestepScheduler`` with its defaults (solver_order 2, algorithm_type "dpmsolver++", solver_type "midpoint",
prediction_type "epsilon", timestep_spacing "linspace", final_sigmas_type "zero", so lower_order_final).  INTEGRATION.md
"DPM-Solver++ scheduler" states the contract; it is a restatement and is not pinned against diffusers.

The step schedule and every scalar coefficient are host work in fp64 (``dpmpp_timesteps``, ``dpmpp_orders``,
``dpmpp_step_coefficients``).  On the device each step is one U-Net call on the (cond, uncond) batch, as in ``DDIMSampler``, and one
fused gfx950 kernel (``af_cfg_dpmpp_step``): guidance combine, data prediction x0 and the update from the sample and x0 of the
current two-step block.
"""
import math

import numpy as np
import torch

from .... import ops
from .ddim import DDIMSampler


def dpmpp_timesteps(S, num_train_timesteps=1000):
    """The S timesteps, descending: linspace(0, T - 1, S + 1) rounded half-to-even, reversed, the trailing 0 dropped."""
    if S < 1:
        raise ValueError(f"DPM-Solver++ needs at least one step, got {S}")
    return np.linspace(0, num_train_timesteps - 1, S + 1).round()[::-1][:-1].copy().astype(np.int64)


def dpmpp_orders(n):
    """Solver order of each of n steps: alternating 1, 2 single-step blocks, ending on order 1 (lower_order_final)."""
    if n < 1:
        raise ValueError(f"DPM-Solver++ needs at least one step, got {n}")
    if n % 2 == 0:
        return [1, 2] * (n // 2 - 1) + [1, 1]
    return [1, 2] * (n // 2) + [1]


def dpmpp_step_coefficients(alphas_cumprod, timesteps, orders):
    """Per step k of a run over ``timesteps`` (descending; after the last comes the final point alpha = 1, sigma = 0) with the given
    orders: (alpha_s, sigma_s, c_base, c0, c1, uses_block_start) in fp64, for x_out = c_base x_base + c0 x0_k + c1 x0_prev where
    x0_k = (x_k - sigma_s e_k) / alpha_s.  Order 1: x_base = x_k, c1 = 0.  Order 2: x_base and x0_prev are the sample and x0 of the
    previous (order-1) step, the start of the two-step block.  The last step is x_out = x0 (c_base 0, c0 1), never through log 0."""
    ac = np.asarray(alphas_cumprod, dtype=np.float64)
    ts = [int(t) for t in timesteps]
    orders = list(orders)
    if len(ts) != len(orders) or not ts:
        raise ValueError(f"{len(ts)} timesteps but {len(orders)} orders")
    for k, o in enumerate(orders):
        if o not in (1, 2) or (o == 2 and (k == 0 or orders[k - 1] != 1)):
            raise ValueError(f"order {o} at step {k}: an order-2 step must follow an order-1 step, orders {orders}")
    if orders[-1] != 1:
        raise ValueError(f"the last step must be order 1, orders {orders}")
    alpha = lambda t: math.sqrt(ac[t])
    sigma = lambda t: math.sqrt(1.0 - ac[t])
    lam = lambda t: math.log(alpha(t)) - math.log(sigma(t))
    out = []
    for k, (t, o) in enumerate(zip(ts, orders)):
        a_s, s_s = alpha(t), sigma(t)
        if k == len(ts) - 1:
            out.append((a_s, s_s, 0.0, 1.0, 0.0, False))
            continue
        t_next = ts[k + 1]
        a_t, s_t = alpha(t_next), sigma(t_next)
        if o == 1:
            h = lam(t_next) - lam(t)
            out.append((a_s, s_s, s_t / s_s, -a_t * math.expm1(-h), 0.0, False))
        else:
            t_blk = ts[k - 1]
            h = lam(t_next) - lam(t_blk)
            r0 = (lam(t) - lam(t_blk)) / h
            d = -a_t * math.expm1(-h)
            out.append((a_s, s_s, s_t / sigma(t_blk), d / (2.0 * r0), d * (1.0 - 1.0 / (2.0 * r0)), True))
    return out


class DPMSolverSampler:
    def __init__(self, model):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps

    def _alphas_cumprod(self):
        ac = self.model.alphas_cumprod.detach().double().cpu().numpy()
        assert ac.shape[0] == self.ddpm_num_timesteps
        return ac

    @staticmethod
    def _guide_scales(n, guidance_scale):
        # the DDIM sampler's annealing rule; one step takes its first scale (guide_scales divides by n - 1)
        return DDIMSampler.guide_scales(n, guidance_scale) if n > 1 else DDIMSampler.guide_scales(2, guidance_scale)[:1]

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, x_T=None, guidance_scale=1.0, unconditional_conditioning=None,
               callback=None, img_callback=None, log_every_t=100, **kwargs):
        """S DPM-Solver++ steps from x_T (drawn with torch.randn when None).  Returns (latents, intermediates) like
        DDIMSampler.sample; intermediates["x_inter"] / ["pred_x0"] start with x_T and record the step with index
        n - 1 - i (0 = last) when index % log_every_t == 0, and the first step."""
        C, H, W = shape
        device = self.model.betas.device
        img = torch.randn((batch_size, C, H, W), device=device) if x_T is None else x_T
        return self._run(dpmpp_timesteps(S, self.ddpm_num_timesteps), img, conditioning, guidance_scale, unconditional_conditioning,
                         callback, img_callback, log_every_t)

    def img2img_steps(self, S, strength):
        """(n, t_first) of an img2img run over the S-step schedule: n = min(int(S * strength), S) steps, the last n of the schedule
        (with the orders of an n-step run), starting from the latent noised to dpmpp_timesteps(S)[S - n]."""
        if not 0 < strength <= 1:
            raise ValueError(f"img2img strength must be in (0, 1], got {strength}")
        n = min(int(S * strength), S)
        if n == 0:
            raise ValueError(f"img2img strength {strength} with {S} steps leaves no denoising step (int({S} * {strength}) = 0)")
        return n, int(dpmpp_timesteps(S, self.ddpm_num_timesteps)[S - n])

    @torch.no_grad()
    def sample_img2img(self, S, strength, batch_size, x_t, conditioning, guidance_scale=1.0, unconditional_conditioning=None,
                       callback=None, img_callback=None, log_every_t=100):
        """Denoise x_t (noised to img2img_steps(S, strength)[1]) through the last n steps of the S-step schedule.
        Returns (latents, intermediates) like sample()."""
        n, _ = self.img2img_steps(S, strength)
        if x_t.shape[0] != batch_size:
            raise ValueError(f"x_t holds {x_t.shape[0]} latents, batch_size is {batch_size}")
        ts = dpmpp_timesteps(S, self.ddpm_num_timesteps)[S - n:]
        return self._run(ts, x_t, conditioning, guidance_scale, unconditional_conditioning, callback, img_callback, log_every_t)

    def _run(self, timesteps, img, cond, guidance_scale, uncond, callback, img_callback, log_every_t):
        n = len(timesteps)
        coefs = dpmpp_step_coefficients(self._alphas_cumprod(), timesteps, dpmpp_orders(n))
        scales = self._guide_scales(n, guidance_scale)
        device = self.model.betas.device
        b = img.shape[0]
        x = img.to(torch.float32).contiguous()
        intermediates = {"x_inter": [x], "pred_x0": [x]}
        x_blk = x0_blk = None
        for i, (t, (a_s, s_s, c_base, c0, c1, uses_blk)) in enumerate(zip(timesteps, coefs)):
            ts = torch.full((b,), int(t), device=device, dtype=torch.long)
            e2, has_uncond = self._eps2(x, cond, ts, scales[i], uncond)
            x_base, x0_prev = (x_blk, x0_blk) if uses_blk else (x, None)
            x_new, x0 = ops.cfg_dpmpp_step(e2, x, x_base, x0_prev, scales[i], a_s, s_s, c_base, c0, c1, has_uncond)
            if not uses_blk:
                x_blk, x0_blk = x, x0          # an order-1 step starts the block of the step after it
            x = x_new
            if callback:
                callback(i)
            if img_callback:
                img_callback(x0, i)
            index = n - i - 1
            if index % log_every_t == 0 or index == n - 1:
                intermediates["x_inter"].append(x)
                intermediates["pred_x0"].append(x0)
        return x, intermediates

    def _eps2(self, x, c, t, guidance_scale, unconditional_conditioning):
        """The U-Net's [e_cond ; e_uncond] (or e_cond alone), batched as DDIMSampler.p_sample_ddim batches it."""
        has_uncond = not (unconditional_conditioning is None or guidance_scale == 1.0)
        if not has_uncond:
            e2 = self.model.apply_model(x, t, c)
        else:
            x_in = torch.cat([x] * 2)
            t_in = torch.cat([t] * 2)
            if isinstance(c, tuple):
                c_c, prompt_in_c, extra_info = c
                c_u, prompt_in_u, _ = unconditional_conditioning
                c2 = (torch.cat([c_c, c_u]), sum([prompt_in_c, prompt_in_u], []), extra_info)  # (cond, uncond) order
            else:
                c2 = torch.cat([c, unconditional_conditioning])
            e2 = self.model.apply_model(x_in, t_in, c2)
        return e2.to(torch.float32).contiguous(), has_uncond
