#!/usr/bin/env python
"""Inpaint against img2img, whole AdaFaceWrapper.forward at full size (seeded random weights): one 512 x 512 image -> 4 outputs, the
same sampler, steps, strength and generator seed; inpaint adds a mask (left half repainted).  One wrapper serves both pipelines
(`pipeline_name` is switched between runs), so both run on the same weights.  After one warm-up pass of each, the two are timed
alternately `reps` times; prints the median and the minimum of each (eager launches).
lcm: the LCM sampler on the unfused SD-1.5 weights (the sampler follows `use_lcm`; a LoRA changes the weights, not the time).
A fifth argument (img2img | inpaint) runs only that pipeline, twice and untimed: the process to put under rocprofv3 --kernel-trace.
                              python tools/e2e_inpaint.py [scheduler: ddim | dpm++ | lcm] [steps] [strength] [reps] [pipeline]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    from PIL import Image

    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper
    scheduler = sys.argv[1] if len(sys.argv) > 1 else "ddim"
    steps = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2] else {"ddim": 50, "dpm++": 20, "lcm": 4}[scheduler]
    strength = float(sys.argv[3]) if len(sys.argv) > 3 else 0.8
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    guidance = 1.5 if scheduler == "lcm" else 6.0
    count = 4
    dev = torch.device("cuda:0")
    w = AdaFaceWrapper(pipeline_name="img2img", device=dev, num_inference_steps=steps,
                       default_scheduler_name="ddim" if scheduler == "lcm" else scheduler)
    w.use_lcm = scheduler == "lcm"
    rng.load_synth_weights(w.ldm.model.diffusion_model, seed=0)
    vae = w.ldm.instantiate_first_stage()
    with torch.no_grad():
        for n, p in vae.named_parameters():
            p.copy_(rng.synth_tensor(n, p.shape, seed=90))
    w.vae = vae
    w.ldm.to(dev)
    w.ldm.model.diffusion_model.prepare()
    img = Image.fromarray(np.random.default_rng(7).integers(0, 256, (512, 512, 3), dtype=np.uint8))
    a = np.zeros((512, 512), dtype=np.uint8)
    a[:, :256] = 255
    mask = Image.fromarray(a)
    pe = rng.synth_input("e2e.pe", (1, 77, 768), seed=7).to(dev)
    ne = rng.synth_input("e2e.ne", (1, 77, 768), seed=8).to(dev)

    def run(pipeline):
        w.pipeline_name = pipeline
        kw = dict(mask_image=mask) if pipeline == "inpaint" else {}
        torch.cuda.synchronize()
        t = time.perf_counter()
        imgs = w(img, None, prompt_embeds=(pe, ne), guidance_scale=guidance, out_image_count=count, ref_img_strength=strength,
                 generator=torch.Generator().manual_seed(1), **kw)
        torch.cuda.synchronize()
        assert len(imgs) == count
        return time.perf_counter() - t

    n, _ = w._sampler().img2img_steps(steps, strength)
    if len(sys.argv) > 5:
        run(sys.argv[5]), run(sys.argv[5])
        print(f"{scheduler}: 2 x {sys.argv[5]} forward, {n} of {steps} steps each")
        return
    run("img2img"), run("inpaint")                              # warm-up: weight packing, kernels
    times = {"img2img": [], "inpaint": []}
    for _ in range(reps):
        for p in times:
            times[p].append(run(p))
    line = " | ".join(f"{p} median {statistics.median(v) * 1e3:.1f} ms min {min(v) * 1e3:.1f} ms" for p, v in times.items())
    print(f"{scheduler}: {n} of {steps} steps (strength {strength}, g {guidance}, {count} outputs 512x512, {reps} reps each) | {line} | "
          f"inpaint / img2img (medians) {statistics.median(times['inpaint']) / statistics.median(times['img2img']):.4f}")


if __name__ == "__main__":
    main()
