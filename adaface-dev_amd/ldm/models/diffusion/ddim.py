"""Host-side mirror of the reference's ``ldm/models/diffusion/ddim.py`` (``DDIMSampler``):
uniform DDIM schedule, classifier-free guidance with the (conditional, unconditional) batch
order and linear guidance annealing (ddim.py:27-67, 133-221, 223-302).

Differences in execution only: the guidance combine and the DDIM update of one step are ONE
fused element-wise kernel (``af_cfg_ddim_step``) on the fp32 latents, the per-step scalar
tables stay on the host (no ``torch.full`` launches), and ``register_buffer`` does not force
tensors onto "cuda" by name (ddim.py:21-25 makes the reference sampler unusable elsewhere).
The loop, the (cond, uncond) batching and the guidance annealing are ``sampling.py``'s, shared
with the DPM-Solver++ and LCM samplers.
"""
import numpy as np
import torch

from .... import ops
from ...modules.diffusionmodules.util import make_ddim_sampling_parameters, make_ddim_timesteps
from .sampling import Sampler, guide_scales


class DDIMSampler(Sampler):
    def __init__(self, model, schedule="linear"):
        super().__init__(model)
        self.schedule = schedule

    def register_buffer(self, name, attr):
        setattr(self, name, attr)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.0, verbose=True):
        if ddim_eta != 0.0:
            raise NotImplementedError("eta > 0 (stochastic DDIM) is not used by the reference path")
        self.ddim_timesteps = make_ddim_timesteps(ddim_discr_method=ddim_discretize, num_ddim_timesteps=ddim_num_steps,
                                                  num_ddpm_timesteps=self.ddpm_num_timesteps, verbose=verbose)
        alphas_cumprod = self.model.alphas_cumprod.detach().float().cpu().numpy()
        assert alphas_cumprod.shape[0] == self.ddpm_num_timesteps
        sig, a, ap = make_ddim_sampling_parameters(alphas_cumprod, self.ddim_timesteps, ddim_eta, verbose=verbose)
        self.register_buffer("ddim_sigmas", sig)
        self.register_buffer("ddim_alphas", a)
        self.register_buffer("ddim_alphas_prev", ap)
        self.register_buffer("ddim_sqrt_one_minus_alphas", np.sqrt(1.0 - a))

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, img_callback=None, eta=0.0, mask=None, x0=None,
               verbose=True, x_T=None, log_every_t=100, guidance_scale=1.0, unconditional_conditioning=None, **kwargs):
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C, H, W = shape
        return self.ddim_sampling(conditioning, (batch_size, C, H, W), callback=callback, img_callback=img_callback,
                                  mask=mask, x0=x0, x_T=x_T, log_every_t=log_every_t, guidance_scale=guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning)

    guide_scales = staticmethod(guide_scales)

    def timesteps(self, S):
        return np.flip(make_ddim_timesteps("uniform", S, self.ddpm_num_timesteps, verbose=False))

    @torch.no_grad()
    def ddim_sampling(self, cond_context, shape, x_T=None, callback=None, timesteps=None, mask=None, x0=None,
                      img_callback=None, log_every_t=100, guidance_scale=1.0, unconditional_conditioning=None, **kwargs):
        img = torch.randn(shape, device=self.model.betas.device) if x_T is None else x_T
        if timesteps is None:
            timesteps = self.ddim_timesteps
        else:
            subset_end = int(min(timesteps / self.ddim_timesteps.shape[0], 1) * self.ddim_timesteps.shape[0]) - 1
            timesteps = self.ddim_timesteps[:subset_end]
        return self._run(np.flip(timesteps), img, cond_context, unconditional_conditioning, guidance_scale, callback, img_callback,
                         log_every_t, self._step(len(timesteps), mask, x0))

    def make_step(self, S, timesteps, generator, blends=None):      # img2img / inpaint steps; sample() runs ddim_sampling
        self.make_schedule(ddim_num_steps=S, ddim_eta=0.0, verbose=False)
        return self._step(len(timesteps), blends=blends)

    def _step(self, n, mask=None, x0=None, blends=None):
        """Step i of a run over the first n timesteps of the schedule: p_sample_ddim at index n - 1 - i, after the LDM mask blend
        (``mask`` / ``x0``) or with the inpaint blend ``blends[i]`` fused into it."""
        def step(i, x, t, c, uc, g):
            if mask is not None:
                assert x0 is not None
                x = (self.model.q_sample(x0, t) * mask + (1.0 - mask) * x).contiguous()
            return self.p_sample_ddim(x, c, t, index=n - 1 - i, guidance_scale=g, unconditional_conditioning=uc,
                                      blend=None if blends is None else blends[i])
        return step

    @torch.no_grad()
    def p_sample_ddim(self, x, c, t, index, guidance_scale=1.0, unconditional_conditioning=None, blend=None, **kwargs):
        """One DDIM step (ddim.py:223-302, eta = 0); ``blend``: an ops.InpaintBlend applied to x_prev in the same kernel."""
        e2, has_uncond = self._eps(x, t, c, unconditional_conditioning, guidance_scale)
        a_t, a_prev = float(self.ddim_alphas[index]), float(self.ddim_alphas_prev[index])
        return ops.cfg_ddim_step(e2, x.to(torch.float32).contiguous(), guidance_scale, a_t, a_prev, has_uncond, blend=blend)
