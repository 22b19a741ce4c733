#!/usr/bin/env python
"""The img2img pipeline end to end at full size through the AdaFaceWrapper surface (seeded random weights): one 512 x 512 input image
-> uint8 upload -> VAE encoder + fused quant_conv / posterior / q_sample -> the last 40 of 50 DDIM steps (strength 0.8) with CFG on the
SD-1.5 U-Net (batch 4 + 4) -> VAE decoder -> 4 PIL images.  Prints the time of each phase after one warm-up pass (eager launches).
                                                          python tools/e2e_img2img.py [steps] [strength] [scheduler: ddim | dpm++]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    from PIL import Image

    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper, img2img_images_u8
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    strength = float(sys.argv[2]) if len(sys.argv) > 2 else 0.8
    scheduler = sys.argv[3] if len(sys.argv) > 3 else "ddim"
    count = 4
    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    w = AdaFaceWrapper(pipeline_name="img2img", device=dev, num_inference_steps=steps, default_scheduler_name=scheduler)
    rng.load_synth_weights(w.ldm.model.diffusion_model, seed=0)
    vae = w.ldm.instantiate_first_stage()
    with torch.no_grad():
        for n, p in vae.named_parameters():
            p.copy_(rng.synth_tensor(n, p.shape, seed=90))
    w.vae = vae
    w.ldm.to(dev)
    w.ldm.model.diffusion_model.prepare()
    torch.cuda.synchronize()
    t_build = time.perf_counter() - t0

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t

    img = Image.fromarray(np.random.default_rng(7).integers(0, 256, (512, 512, 3), dtype=np.uint8))
    pe = rng.synth_input("e2e.pe", (1, 77, 768), seed=7).to(dev)
    ne = rng.synth_input("e2e.ne", (1, 77, 768), seed=8).to(dev)
    cond = (pe.repeat(count, 1, 1), [""] * count, {})
    uncond = (ne.repeat(count, 1, 1), [""] * count, {})
    sampler = w._sampler()
    n, t_first = sampler.img2img_steps(steps, strength)
    for it in range(2):                                      # first pass packs weights / warms kernels
        x_t, t_enc = timed(lambda: w.ldm.img2img_latents(img2img_images_u8(img, count).to(dev), count, t_first,
                                                         generator=torch.Generator().manual_seed(1)))
        lat, t_ddim = timed(lambda: sampler.sample_img2img(steps, strength, count, x_t, cond, guidance_scale=6.0,
                                                           unconditional_conditioning=uncond)[0])
        _, t_vae = timed(lambda: vae.decode(lat / 0.18215))
    imgs, t_all = timed(lambda: w(img, None, prompt_embeds=(pe, ne), guidance_scale=6.0, out_image_count=count, ref_img_strength=strength,
                                  generator=torch.Generator().manual_seed(1)))
    print(f"build+weights {t_build:.1f} s | image upload + VAE encode + latents (1 image 512x512) {t_enc * 1e3:.1f} ms | "
          f"{n} of {steps} {scheduler} steps (strength {strength}, t_first {t_first}, U-Net batch {2 * count}, eager) {t_ddim * 1e3:.1f} ms = "
          f"{t_ddim / n * 1e3:.2f} ms/step | VAE decode x{count} {t_vae * 1e3:.1f} ms | whole img2img forward() incl. PIL {t_all * 1e3:.1f} ms | "
          f"{len(imgs)} images {imgs[0].size}, latents finite={bool(torch.isfinite(lat).all())}")


if __name__ == "__main__":
    main()
