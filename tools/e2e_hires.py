#!/usr/bin/env python
"""Two-pass high-resolution text2img against the direct one-pass run, whole AdaFaceWrapper.forward at full size (seeded random
weights): 4 outputs, first pass at 512 x 512, then `hires_size` (default 1024 x 768) at `strength` of the same step count; the direct
run samples all steps from noise at the target size.  One wrapper serves both.  After one warm-up of each, the two are timed
alternately `reps` times (eager launches); prints the median and minimum of each and, for the two-pass run, the medians of its four
parts (first pass, the af_latent_resize_q_sample launch with its randn, second pass, decode), each closed by a device synchronise.
Then the kernel alone against the torch form on the GPU at the same shape (F.interpolate, two scalings, an add), device events
over `iters` back-to-back calls, alternated 5 times, both modes.
                              python tools/e2e_hires.py [scheduler: ddim | dpm++ | lcm] [steps] [strength] [reps] [W] [H]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def timed(obj, name, bucket):
    """Replace obj.name by a version that adds its synchronised wall time to bucket[name]."""
    fn = getattr(obj, name)

    def wrapper(*a, **kw):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn(*a, **kw)
        torch.cuda.synchronize()
        bucket[name] = bucket.get(name, 0.0) + time.perf_counter() - t
        return out

    setattr(obj, name, wrapper)


def kernel_alone(dev, shape, size_hw, iters=200):
    from adaface_dev_amd import ops
    x = torch.randn(shape, device=dev)
    n = torch.randn(shape[:2] + tuple(size_hw), device=dev)
    sa, sb = 0.8, 0.6

    def events(fn):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / iters

    for mode in ("bilinear", "bicubic"):
        fused = lambda: ops.latent_resize_q_sample(x, size_hw, mode, n, sa, sb)
        plain = lambda: sa * F.interpolate(x, size=size_hw, mode=mode, align_corners=False) + sb * n
        diff = float((fused() - plain()).abs().max())
        tf, tp = [], []
        for _ in range(5):
            tf.append(events(fused))
            tp.append(events(plain))
        byts = 4 * (x.numel() + 2 * n.numel())
        print(f"kernel alone, {mode} {tuple(shape)} -> {tuple(size_hw)} ({byts / 1e6:.2f} MB moved): af_latent_resize_q_sample median "
              f"{statistics.median(tf):.2f} us min {min(tf):.2f} us per call | torch interpolate + scale + scale + add median "
              f"{statistics.median(tp):.2f} us min {min(tp):.2f} us | max |fused - torch| {diff:.2e}")


def main():
    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper
    scheduler = sys.argv[1] if len(sys.argv) > 1 else "dpm++"
    steps = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2] else {"ddim": 50, "dpm++": 20, "lcm": 4}[scheduler]
    strength = float(sys.argv[3]) if len(sys.argv) > 3 else 0.7
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    W = int(sys.argv[5]) if len(sys.argv) > 5 else 1024
    H = int(sys.argv[6]) if len(sys.argv) > 6 else 768
    guidance = 1.5 if scheduler == "lcm" else 6.0
    count = 4
    dev = torch.device("cuda:0")
    w = AdaFaceWrapper(pipeline_name="text2img", device=dev, num_inference_steps=steps,
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
    pe = rng.synth_input("e2e.pe", (1, 77, 768), seed=7).to(dev)
    ne = rng.synth_input("e2e.ne", (1, 77, 768), seed=8).to(dev)
    noise_lo = rng.synth_input("e2e.noise512", (count, 4, 64, 64), seed=9).to(dev)
    noise_hi = rng.synth_input("e2e.noisehi", (count, 4, H // 8, W // 8), seed=10).to(dev)
    parts = {}
    make_sampler = w._sampler

    def sampler():
        s = make_sampler()
        timed(s, "sample", parts)
        timed(s, "sample_img2img", parts)
        return s

    w._sampler = sampler
    timed(w.ldm, "hires_latents", parts)
    timed(w, "_to_pil", parts)

    def run(two_pass):
        parts.clear()
        kw = dict(hires_size=(W, H), hires_strength=strength) if two_pass else {}
        torch.cuda.synchronize()
        t = time.perf_counter()
        imgs = w(noise_lo if two_pass else noise_hi, None, prompt_embeds=(pe, ne), guidance_scale=guidance, out_image_count=count,
                 generator=torch.Generator().manual_seed(1), **kw)
        torch.cuda.synchronize()
        assert len(imgs) == count and imgs[0].size == (W, H)
        return time.perf_counter() - t, dict(parts)

    n2, _ = make_sampler().img2img_steps(steps, strength)
    run(True), run(False)                                       # warm-up: weight packing, kernels at both sizes
    whole = {True: [], False: []}
    split = {k: [] for k in ("sample", "hires_latents", "sample_img2img", "_to_pil")}
    for _ in range(reps):
        for two_pass in (True, False):
            t, p = run(two_pass)
            whole[two_pass].append(t)
            if two_pass:
                for k in split:
                    split[k].append(p[k])
    med = lambda v: statistics.median(v) * 1e3
    print(f"{scheduler}: {count} outputs, {steps} steps at 512x512 + {n2} of {steps} at {W}x{H} (strength {strength}, g {guidance}, "
          f"{reps} reps each, alternated) | two-pass median {med(whole[True]):.1f} ms min {min(whole[True]) * 1e3:.1f} ms | direct "
          f"{steps} steps at {W}x{H} median {med(whole[False]):.1f} ms min {min(whole[False]) * 1e3:.1f} ms | two-pass / direct "
          f"(medians) {med(whole[True]) / med(whole[False]):.4f}")
    print(f"two-pass parts (medians): first pass {med(split['sample']):.1f} ms | randn + af_latent_resize_q_sample "
          f"{med(split['hires_latents']):.3f} ms | second pass {med(split['sample_img2img']):.1f} ms | decode to PIL "
          f"{med(split['_to_pil']):.1f} ms")
    kernel_alone(dev, (count, 4, 64, 64), (H // 8, W // 8))


if __name__ == "__main__":
    main()
