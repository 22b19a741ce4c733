"""The sampling loop shared by ``DDIMSampler``, ``DPMSolverSampler`` and ``LCMSampler``, and the rules they have in common: the
(cond, uncond) batching of one U-Net call, the reference's guidance annealing and the img2img step count.

A sampler subclasses ``Sampler`` and gives only what makes it different: its descending S-step schedule (``timesteps``), its
guidance policy (``guidance_scales`` and ``runs_uncond``) and, per run, its step (``make_step``): the U-Net call and the fused
gfx950 kernel of one step, with whatever state the steps of a run share.
"""
import math

import torch

from .... import ops


def guide_scales(n, guidance_scale):
    """The scale used at each of n steps (the reference's ddim.py:166-181, 216-219): annealed linearly from max_g to min_g for a
    (max_g, min_g) pair, max(2, g) throughout for a scalar g.  One step takes the first scale, max_g (the rule divides by n - 1)."""
    if isinstance(guidance_scale, (list, tuple)):
        max_g, min_g = guidance_scale
    else:
        min_g = max_g = max(2.0, guidance_scale)
    if n == 1:
        return [max_g]
    max_anneal = n - 1
    delta = (max_g - min_g) / max_anneal
    scales, g = [], max_g
    for i in range(n):
        scales.append(g)
        g = g - delta if i <= max_anneal else 1
    return scales


class Sampler:
    def __init__(self, model):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps

    def timesteps(self, S):
        """The timesteps of an S-step run, descending."""
        raise NotImplementedError

    def make_step(self, S, timesteps, generator, blends=None):
        """step(i, x, t, cond, uncond, guidance_scale) -> (x_next, x0) for step i of a run over ``timesteps``, the last
        len(timesteps) of the S-step schedule.  ``generator`` draws whatever the steps draw.  ``blends`` (inpainting): one
        ops.InpaintBlend per step, which the step's fused kernel applies to x_next."""
        raise NotImplementedError

    def guidance_scales(self, n, guidance_scale):
        """The scale of each of n steps: the reference's annealing rule."""
        return guide_scales(n, guidance_scale)

    @staticmethod
    def runs_uncond(unconditional_conditioning, scale):
        """Whether a step at this scale runs the (cond, uncond) batch: an uncond is given and the scale is not 1."""
        return unconditional_conditioning is not None and scale != 1.0

    def _eps(self, x, t, c, unconditional_conditioning, scale):
        """(e2, has_uncond): the U-Net's [e_cond ; e_uncond] on the (cond, uncond) batch (the reference's ddim.py:223-253) when
        runs_uncond says so, else e_cond alone; fp32 and contiguous, as the fused step kernels take it."""
        has_uncond = self.runs_uncond(unconditional_conditioning, scale)
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

    def _alphas_cumprod(self):
        ac = self.model.alphas_cumprod.detach().double().cpu().numpy()
        assert ac.shape[0] == self.ddpm_num_timesteps
        return ac

    def img2img_steps(self, S, strength):
        """(n, t_first) of an img2img run over the S-step schedule (diffusers' StableDiffusionImg2ImgPipeline.get_timesteps):
        n = min(int(S * strength), S) steps, the last n of the schedule, starting from the latent noised to the first of them."""
        if not 0 < strength <= 1:
            raise ValueError(f"img2img strength must be in (0, 1], got {strength}")
        n = min(int(S * strength), S)
        if n == 0:
            raise ValueError(f"img2img strength {strength} with {S} steps leaves no denoising step (int({S} * {strength}) = 0)")
        return n, int(self.timesteps(S)[-n])

    def inpaint_blends(self, timesteps, z, noise, mask):
        """The blend of each step of an inpaint run over ``timesteps`` (INTEGRATION.md "Inpainting" rule 4): after step i the
        known region is z noised with ``noise`` to timesteps[i + 1], (sa, sb) = (sqrt(abar), sqrt(1 - abar)) in fp64, and z
        itself after the last step."""
        ac = self._alphas_cumprod()
        ts = [int(t) for t in timesteps]
        nxt = [ops.InpaintBlend(z, noise, mask, math.sqrt(ac[t]), math.sqrt(1.0 - ac[t])) for t in ts[1:]]
        return nxt + [ops.InpaintBlend(z, None, mask)]

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, x_T=None, guidance_scale=1.0, unconditional_conditioning=None,
               callback=None, img_callback=None, log_every_t=100, generator=None, **kwargs):
        """S steps from x_T (drawn with torch.randn when None); ``generator`` goes to make_step (LCM draws from it, DDIM and
        DPM-Solver++ ignore it).  Returns (latents, intermediates) as _run does."""
        C, H, W = shape
        img = torch.randn((batch_size, C, H, W), device=self.model.betas.device) if x_T is None else x_T
        ts = self.timesteps(S)
        return self._run(ts, img, conditioning, unconditional_conditioning, guidance_scale, callback, img_callback, log_every_t,
                         self.make_step(S, ts, generator))

    @torch.no_grad()
    def sample_img2img(self, S, strength, batch_size, x_t, conditioning, guidance_scale=1.0, unconditional_conditioning=None,
                       callback=None, img_callback=None, log_every_t=100, generator=None):
        """Denoise x_t (noised to img2img_steps(S, strength)[1], e.g. by LatentDiffusion.img2img_latents) through the last n steps
        of the S-step schedule, with the guidance scales of an n-step run.  Returns (latents, intermediates) like sample()."""
        n, _ = self.img2img_steps(S, strength)
        if x_t.shape[0] != batch_size:
            raise ValueError(f"x_t holds {x_t.shape[0]} latents, batch_size is {batch_size}")
        ts = self.timesteps(S)[-n:]
        return self._run(ts, x_t, conditioning, unconditional_conditioning, guidance_scale, callback, img_callback, log_every_t,
                         self.make_step(S, ts, generator))

    @torch.no_grad()
    def sample_inpaint(self, S, strength, batch_size, x_start, z, noise, mask, conditioning, guidance_scale=1.0,
                       unconditional_conditioning=None, callback=None, img_callback=None, log_every_t=100, generator=None):
        """sample_img2img's steps from x_start (e.g. LatentDiffusion.inpaint_latents), each followed in its kernel by the mask blend
        of inpaint_blends: where ``mask`` (fp32 {0, 1} [B_mask, 1, h, w], 1 = repaint) is 0, the latent handed on is the image
        latent z [B_img, 4, h, w] noised with ``noise`` (the start noise [batch_size, 4, h, w]) to the next timestep, and z itself
        after the last step.  Output b uses z[b % B_img] and mask[b % B_mask].  Returns (latents, intermediates) like sample()."""
        n, _ = self.img2img_steps(S, strength)
        for name, t in (("x_start", x_start), ("noise", noise)):
            if t.shape[0] != batch_size:
                raise ValueError(f"{name} holds {t.shape[0]} latents, batch_size is {batch_size}")
        ts = self.timesteps(S)[-n:]
        blends = self.inpaint_blends(ts, z.to(torch.float32).contiguous(), noise.to(torch.float32).contiguous(),
                                     mask.to(torch.float32).contiguous())
        return self._run(ts, x_start, conditioning, unconditional_conditioning, guidance_scale, callback, img_callback, log_every_t,
                         self.make_step(S, ts, generator, blends))

    def _run(self, timesteps, img, cond, uncond, guidance_scale, callback, img_callback, log_every_t, step):
        """step() over ``timesteps`` (descending) from img.  Returns (latents, intermediates); intermediates["x_inter"] /
        ["pred_x0"] start with img and record the step with index n - 1 - i (0 = last) when index % log_every_t == 0, and the
        first step."""
        n = len(timesteps)
        scales = self.guidance_scales(n, guidance_scale)
        device = self.model.betas.device
        x = img.to(torch.float32).contiguous()
        intermediates = {"x_inter": [x], "pred_x0": [x]}
        for i, t in enumerate(timesteps):
            ts = torch.full((x.shape[0],), int(t), device=device, dtype=torch.long)
            x, x0 = step(i, x, ts, cond, uncond, scales[i])
            if callback:
                callback(i)
            if img_callback:
                img_callback(x0, i)
            index = n - i - 1
            if index % log_every_t == 0 or index == n - 1:
                intermediates["x_inter"].append(x)
                intermediates["pred_x0"].append(x0)
        return x, intermediates
