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


class LCMSampler:
    def __init__(self, model):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps

    def _alphas_cumprod(self):
        ac = self.model.alphas_cumprod.detach().double().cpu().numpy()
        assert ac.shape[0] == self.ddpm_num_timesteps
        return ac

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, x_T=None, guidance_scale=1.0, unconditional_conditioning=None,
               callback=None, img_callback=None, log_every_t=100, generator=None, **kwargs):
        """S LCM steps from x_T (drawn with torch.randn when None).  Returns (latents, intermediates) like DDIMSampler.sample;
        intermediates["x_inter"] / ["pred_x0"] (the denoised sample d) start with x_T and record the step with index n - 1 - i
        (0 = last) when index % log_every_t == 0, and the first step.  ``generator`` draws the re-noising of every step but the last,
        in step order, on its own device (the default CUDA generator when None)."""
        C, H, W = shape
        device = self.model.betas.device
        img = torch.randn((batch_size, C, H, W), device=device) if x_T is None else x_T
        return self._run(lcm_timesteps(S, self.ddpm_num_timesteps), img, conditioning, guidance_scale, unconditional_conditioning,
                         callback, img_callback, log_every_t, generator)

    def img2img_steps(self, S, strength):
        """(n, t_first) of an img2img run over the S-step schedule: n = min(int(S * strength), S) steps, the last n of the schedule,
        starting from the latent noised to lcm_timesteps(S)[S - n]."""
        ts = lcm_timesteps(S, self.ddpm_num_timesteps)
        if not 0 < strength <= 1:
            raise ValueError(f"img2img strength must be in (0, 1], got {strength}")
        n = min(int(S * strength), S)
        if n == 0:
            raise ValueError(f"img2img strength {strength} with {S} steps leaves no denoising step (int({S} * {strength}) = 0)")
        return n, int(ts[S - n])

    @torch.no_grad()
    def sample_img2img(self, S, strength, batch_size, x_t, conditioning, guidance_scale=1.0, unconditional_conditioning=None,
                       callback=None, img_callback=None, log_every_t=100, generator=None):
        """Denoise x_t (noised to img2img_steps(S, strength)[1]) through the last n steps of the S-step schedule.
        Returns (latents, intermediates) like sample()."""
        n, _ = self.img2img_steps(S, strength)
        if x_t.shape[0] != batch_size:
            raise ValueError(f"x_t holds {x_t.shape[0]} latents, batch_size is {batch_size}")
        ts = lcm_timesteps(S, self.ddpm_num_timesteps)[S - n:]
        return self._run(ts, x_t, conditioning, guidance_scale, unconditional_conditioning, callback, img_callback, log_every_t,
                         generator)

    def _run(self, timesteps, img, cond, guidance_scale, uncond, callback, img_callback, log_every_t, generator):
        n = len(timesteps)
        coefs = lcm_step_coefficients(self._alphas_cumprod(), timesteps)
        device = self.model.betas.device
        gdev = generator.device if generator is not None else device
        b = img.shape[0]
        x = img.to(torch.float32).contiguous()
        intermediates = {"x_inter": [x], "pred_x0": [x]}
        has_uncond = unconditional_conditioning_used(uncond, guidance_scale)
        for i, (t, (sa, sb, c_out, c_skip, sa_next, sb_next)) in enumerate(zip(timesteps, coefs)):
            ts = torch.full((b,), int(t), device=device, dtype=torch.long)
            e2 = self._eps2(x, cond, ts, uncond if has_uncond else None)
            if i < n - 1:
                noise = torch.randn(x.shape, generator=generator, device=gdev).to(device)
                x, d = ops.cfg_lcm_step(e2, x, noise, guidance_scale, sa, sb, c_out, c_skip, sa_next, sb_next, has_uncond)
            else:
                x, d = ops.cfg_lcm_step(e2, x, None, guidance_scale, sa, sb, c_out, c_skip, has_uncond=has_uncond)
            if callback:
                callback(i)
            if img_callback:
                img_callback(d, i)
            index = n - i - 1
            if index % log_every_t == 0 or index == n - 1:
                intermediates["x_inter"].append(x)
                intermediates["pred_x0"].append(d)
        return x, intermediates

    def _eps2(self, x, c, t, unconditional_conditioning):
        """The U-Net's [e_cond ; e_uncond] (or e_cond alone when unconditional_conditioning is None), batched as
        DDIMSampler.p_sample_ddim batches it."""
        if unconditional_conditioning is None:
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
        return e2.to(torch.float32).contiguous()


def unconditional_conditioning_used(unconditional_conditioning, guidance_scale):
    """diffusers' rule for LCM-LoRA: the (cond, uncond) batch runs only when an uncond is given and the guidance scale is above 1."""
    return unconditional_conditioning is not None and guidance_scale > 1.0
