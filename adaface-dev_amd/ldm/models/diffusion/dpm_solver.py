"""DPM-Solver++ sampling (Lu et al., 2022): the reference wrapper's ``"dpm++"`` scheduler, restated from diffusers'
``DPMSolverSinglestepScheduler`` with its defaults (solver_order 2, algorithm_type "dpmsolver++", solver_type "midpoint",
prediction_type "epsilon", timestep_spacing "linspace", final_sigmas_type "zero", so lower_order_final).  INTEGRATION.md
"DPM-Solver++ scheduler" states the contract; it is a restatement and is not pinned against diffusers.

The step schedule and every scalar coefficient are host work in fp64 (``dpmpp_timesteps``, ``dpmpp_orders``,
``dpmpp_step_coefficients``); img2img runs the last n timesteps of the S-step schedule with the orders of an n-step run.  The loop,
the (cond, uncond) batching and the guidance rule are ``DDIMSampler``'s (``sampling.py``).  On the device each step is one U-Net call
and one fused gfx950 kernel (``af_cfg_dpmpp_step``): guidance combine, data prediction x0 and the update from the sample and x0 of
the current two-step block.
"""
import math

import numpy as np
import torch

from .... import ops
from .sampling import Sampler


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


class DPMSolverSampler(Sampler):
    def timesteps(self, S):
        return dpmpp_timesteps(S, self.ddpm_num_timesteps)

    def make_step(self, S, timesteps, generator, blends=None):
        coefs = dpmpp_step_coefficients(self._alphas_cumprod(), timesteps, dpmpp_orders(len(timesteps)))
        x_blk = x0_blk = None

        def step(i, x, t, c, uc, g):
            nonlocal x_blk, x0_blk
            a_s, s_s, c_base, c0, c1, uses_blk = coefs[i]
            e2, has_uncond = self._eps(x, t, c, uc, g)
            x_base, x0_prev = (x_blk, x0_blk) if uses_blk else (x, None)
            x_new, x0 = ops.cfg_dpmpp_step(e2, x, x_base, x0_prev, g, a_s, s_s, c_base, c0, c1, has_uncond,
                                           blend=None if blends is None else blends[i])
            if not uses_blk:
                x_blk, x0_blk = x, x0          # an order-1 step starts the block of the step after it
            return x_new, x0
        return step
