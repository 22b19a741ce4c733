#!/usr/bin/env python
"""Timings behind profiles/animatediff.txt (MI355X): af_temporal_attention alone at SD-1.5's four levels against the torch device
composition of the same attention, and one 16-frame 512 x 512 U-Net step with and without a motion module.  Medians of --reps runs after
--warmup, with min / max; the arms of a comparison run in one process, alternated.  Device events; bytes are computed from the shapes.

    python tools/bench_animatediff.py kernel [--out profiles/animatediff.txt]
    python tools/bench_animatediff.py step   [--out profiles/animatediff.txt]     (appends)
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

LEVELS = [(320, 64 * 64), (640, 32 * 32), (1280, 16 * 16), (1280, 8 * 8)]      # (channels, pixels) of a 512 x 512 image's four U-Net levels
FRAMES, VIDEOS, HEADS = 16, 2, 8


def _time(fns, reps, warmup):
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {n: [] for n in fns}
    for _ in range(reps):
        for n, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ts[n].append(e0.elapsed_time(e1))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in ts.items()}


def _emit(out, line):
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _torch_composition(qkv, B, nf, HW, heads, d):
    """permute + scaled_dot_product_attention + permute on the device: what the layer costs without the kernel."""
    C = heads * d
    x = qkv.reshape(B, nf, HW, 3, heads, d)
    q, k, v = (x[:, :, :, i].permute(0, 2, 3, 1, 4).contiguous() for i in range(3))            # [B, HW, heads, F, d]
    o = F.scaled_dot_product_attention(q, k, v)
    return o.permute(0, 3, 1, 2, 4).reshape(B * nf * HW, C)


def kernel(args, dev):
    from adaface_dev_amd import ops
    _emit(args.out, f"# af_temporal_attention, F = {FRAMES}, B = {VIDEOS}, {HEADS} heads; median of {args.reps} (min .. max) ms; "
                    "GB/s = 2 (3C + C) bytes per token row over the median")
    for C, HW in LEVELS:
        d = C // HEADS
        rows = VIDEOS * FRAMES * HW
        qkv = (torch.randn((rows, 3 * C), generator=torch.Generator().manual_seed(C + HW)) * 0.5).half().to(dev)
        got = ops.temporal_attention(qkv, B=VIDEOS, F=FRAMES, HW=HW, heads=HEADS, d=d)
        ref = _torch_composition(qkv, VIDEOS, FRAMES, HW, HEADS, d)
        diff = float((got.float() - ref.float()).abs().max())
        r = _time({"hip": lambda: ops.temporal_attention(qkv, B=VIDEOS, F=FRAMES, HW=HW, heads=HEADS, d=d),
                   "torch": lambda: _torch_composition(qkv, VIDEOS, FRAMES, HW, HEADS, d)}, args.reps, args.warmup)
        gbs = 2.0 * 4 * C * rows / (r["hip"][0] * 1e-3) / 1e9
        _emit(args.out, f"C={C:5d} HW={HW:5d} d={d:4d} rows={rows:7d}  af_temporal_attention {r['hip'][0]:8.4f} ({r['hip'][1]:.4f} .. {r['hip'][2]:.4f})  "
                        f"{gbs:8.1f} GB/s   torch permute+sdpa+permute {r['torch'][0]:8.4f} ({r['torch'][1]:.4f} .. {r['torch'][2]:.4f})   "
                        f"max |difference| {diff:.2e}")


def _synthetic_motion_module(unet_cfg):
    """A v2 module at the U-Net's widths with N(0, 1 / fan_in) weights drawn by torch (a benchmark needs shapes, not the tests' Philox values)."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.modules.motion_module import MotionModule, TemporalTransformer, motion_placement
    mc, mult = unet_cfg["model_channels"], unet_cfg["channel_mult"]
    g = torch.Generator().manual_seed(3)
    sd = {}
    with rng.skip_default_init():             # every parameter is overwritten below
        for prefix in motion_placement(True):
            i = int(prefix.split(".")[1]) if not prefix.startswith("mid") else 3
            C = mc * (mult[3 - i] if prefix.startswith("up") else mult[i])
            for k, v in TemporalTransformer(C).state_dict().items():
                if k.endswith("pos_encoder.pe"):
                    t = v
                elif v.dim() == 1:
                    t = torch.ones_like(v) if k.endswith("weight") else torch.zeros_like(v)
                else:
                    t = torch.randn(v.shape, generator=g) / v.shape[1] ** 0.5
                sd[f"{prefix}.temporal_transformer.{k}"] = t
        return MotionModule(sd)


def step(args, dev):
    from adaface_dev_amd import SD15_UNET_CONFIG, rng
    from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    with rng.skip_default_init():
        unet = UNetModel(**SD15_UNET_CONFIG)
    unet = unet.to(dev).eval()
    rng.load_synth_weights(unet, seed=0, on_device=True)
    mm = _synthetic_motion_module(SD15_UNET_CONFIG).to(dev)
    x = torch.randn((FRAMES, 4, 64, 64), generator=torch.Generator().manual_seed(1)).to(dev)
    t = torch.full((FRAMES,), 500, dtype=torch.long, device=dev)
    ctx = torch.randn((1, 77, 768), generator=torch.Generator().manual_seed(2)).repeat(FRAMES, 1, 1).to(dev)

    def run(motion):
        def f():
            unet.set_motion(mm if motion else None, FRAMES if motion else 0)
            try:
                with torch.no_grad():
                    return unet(x, t, ctx, extra_info={})
            finally:
                unet.set_motion(None)
        return f
    assert bool(torch.isfinite(run(True)()).all())
    r = _time({"image": run(False), "video": run(True)}, args.reps, args.warmup)
    _emit(args.out, f"# one U-Net call, SD-1.5 width, {FRAMES} frames of 512 x 512 (batch {FRAMES}, no CFG pair), eager launches; median of {args.reps} (min .. max) ms")
    _emit(args.out, f"without a motion module {r['image'][0]:9.3f} ({r['image'][1]:.3f} .. {r['image'][2]:.3f})")
    _emit(args.out, f"with a v2 motion module {r['video'][0]:9.3f} ({r['video'][1]:.3f} .. {r['video'][2]:.3f})   "
                    f"+{r['video'][0] - r['image'][0]:.3f} ms for 21 temporal transformers")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "step"])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    {"kernel": kernel, "step": step}[a.what](a, torch.device("cuda:0"))
