"""LCM sampling (Luo et al., 2023, "Latent Consistency Models"; LCM-LoRA): the reference wrapper's ``use_lcm`` scheduler, restated
from diffusers' ``LCMScheduler`` with the settings ``from_config`` takes from the SD-1.5 DDIM config (original_inference_steps 50,
timestep_scaling 10, prediction_type "epsilon", no clipping or thresholding, timestep_spacing "leading" unused).  INTEGRATION.md
"LCM-LoRA" states the contract; it is a restatement and is not pinned against diffusers.

The schedule and every scalar are host work in fp64 (``lcm_timesteps``, ``lcm_boundary_scalings``, ``lcm_step_coefficients``).  On the
device each step is one U-Net call -- on the (cond, uncond) batch only when an uncond is given and the guidance scale is above 1,
diffusers' rule -- and one fused gfx950 kernel (``af_cfg_lcm_step``): guidance combine, x0, the boundary-condition blend and the
re-noising to the next timestep.  The guidance scale is constant over the steps: unlike ``DDIMSampler`` / ``DPMSolverSampler`` it is
neither annealed nor clamped to ``max(2, g)``, which would rule out LCM's usual g = 1-2.
"""
import math

import numpy as np
import torch

from .... import ops
from .sampling import Sampler

ORIGINAL_INFERENCE_STEPS = 50
TIMESTEP_SCALING = 10.0
SIGMA_DATA = 0.5


def lcm_timesteps(S, num_train_timesteps=1000, original_inference_steps=ORIGINAL_INFERENCE_STEPS):
    """The S timesteps, descending: the skipped "origin" schedule (k, 2k, ..., 50k) - 1 with k = T / 50 (19 ... 999), reversed, at
    the indices floor(linspace(0, 50, S, endpoint=False)).  S = 4 gives 999, 759, 499, 259."""
    if not 1 <= S <= original_inference_steps:
        raise ValueError(f"LCM takes 1 to {original_inference_steps} steps (original_inference_steps), got {S}")
    k = num_train_timesteps // original_inference_steps
    origin = np.arange(1, original_inference_steps + 1, dtype=np.int64) * k - 1
    idx = np.floor(np.linspace(0, original_inference_steps, S, endpoint=False)).astype(np.int64)
    return origin[::-1][idx].copy()


def lcm_boundary_scalings(t, timestep_scaling=TIMESTEP_SCALING, sigma_data=SIGMA_DATA):
    """(c_skip, c_out) of timestep t in fp64: u = 10 t, c_skip = sigma_data^2 / (u^2 + sigma_data^2), c_out = u / sqrt(u^2 + sigma_data^2)."""
    u = float(t) * timestep_scaling
    return sigma_data ** 2 / (u * u + sigma_data ** 2), u / math.sqrt(u * u + sigma_data ** 2)


def lcm_step_coefficients(alphas_cumprod, timesteps):
    """Per step i of a run over ``timesteps`` (descending): (sqrt_a, sqrt_1ma, c_out, c_skip, sqrt_a_next, sqrt_1ma_next) in fp64 for
    x0 = (x - sqrt_1ma e) / sqrt_a, d = c_out x0 + c_skip x, x_next = sqrt_a_next d + sqrt_1ma_next n.  The next values are taken at
    timesteps[i + 1]; the last step returns d and its next values are None."""
    ac = np.asarray(alphas_cumprod, dtype=np.float64)
    ts = [int(t) for t in timesteps]
    if not ts:
        raise ValueError("an LCM run needs at least one timestep")
    out = []
    for i, t in enumerate(ts):
        c_skip, c_out = lcm_boundary_scalings(t)
        nxt = (None, None) if i == len(ts) - 1 else (math.sqrt(ac[ts[i + 1]]), math.sqrt(1.0 - ac[ts[i + 1]]))
        out.append((math.sqrt(ac[t]), math.sqrt(1.0 - ac[t]), c_out, c_skip) + nxt)
    return out


class LCMSampler(Sampler):
    def timesteps(self, S):
        return lcm_timesteps(S, self.ddpm_num_timesteps)

    def guidance_scales(self, n, guidance_scale):
        return [guidance_scale] * n

    @staticmethod
    def runs_uncond(unconditional_conditioning, scale):
        """diffusers' rule for LCM-LoRA: the (cond, uncond) batch runs only when an uncond is given and the guidance scale is above 1."""
        return unconditional_conditioning is not None and scale > 1.0

    def make_step(self, S, timesteps, generator, blends=None):
        """``generator`` draws the re-noising of every step but the last, in step order, on its own device (the default CUDA
        generator when None)."""
        n = len(timesteps)
        coefs = lcm_step_coefficients(self._alphas_cumprod(), timesteps)
        device = self.model.betas.device
        gdev = generator.device if generator is not None else device

        def step(i, x, t, c, uc, g):
            sa, sb, c_out, c_skip, sa_next, sb_next = coefs[i]
            e2, has_uncond = self._eps(x, t, c, uc, g)
            blend = None if blends is None else blends[i]
            if i < n - 1:
                noise = torch.randn(x.shape, generator=generator, device=gdev).to(device)
                return ops.cfg_lcm_step(e2, x, noise, g, sa, sb, c_out, c_skip, sa_next, sb_next, has_uncond, blend=blend)
            return ops.cfg_lcm_step(e2, x, None, g, sa, sb, c_out, c_skip, has_uncond=has_uncond, blend=blend)
        return step
