#!/usr/bin/env python
"""GFPGAN face restoration at full size (GFPGANv1Clean at the v1.4 configuration, 512 x 512 crops, seeded random weights: no checkpoint is
available): `net.hip` on 1 and on 4 crops and the whole `FaceRestorer.restore_u8` of a 1024 x 1024 photo with 1 and 4 faces (a stub detector
with fixed landmarks: the detector network is the caller's and is not timed), alternated in the same run with the module's own torch `forward`
in fp16 on the same GPU.  Device events around `reps` calls after a warm-up (weight packing, scratch allocation), median and minimum.
Then `af_modulate_weights` alone, layer by layer (`iters` back-to-back calls each): its share of the walk and its achieved bytes per second
(fp32 master weights and wsq read, fp16 per-sample weights written), which is what a memory-bound kernel is judged by.
                              python tools/e2e_gfpgan.py [reps] [iters]
With reps = 0 only one warmed-up `net.hip` of one crop runs (for `rocprofv3 --kernel-trace --stats -- python tools/e2e_gfpgan.py 0`)."""
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main():
    from adaface_dev_amd import ops
    from adaface_dev_amd.adaface.gfpgan import FaceRestorer, GFPGANv1Clean, ffhq_template
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = GFPGANv1Clean().eval()
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("style_conv1.weight") or (".style_convs." in name and name.count(".") == 3 and name.endswith(".weight")):
                p.fill_(0.1)                       # noise weights (zero by default)
    net = net.to(dev)
    half = GFPGANv1Clean().eval()
    half.load_state_dict(net.state_dict())
    half = half.to(dev).half()
    g = np.random.default_rng(0)
    crops = torch.zeros((4, 512, 512, 8), dtype=torch.float16, device=dev)
    crops[..., :3] = torch.from_numpy(g.uniform(-1, 1, (4, 512, 512, 3))).to(dev).half()
    nchw = crops[..., :3].permute(0, 3, 1, 2).contiguous()
    out = net.hip(crops[:1])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all())
    if reps == 0:
        for _ in range(2):                         # three walks in all: the last one is the trace's steady state
            net.hip(crops[:1])
        torch.cuda.synchronize()
        return
    with torch.no_grad():
        ref = half(nchw[:1])
    d = float((out[..., :3].float().permute(0, 3, 1, 2) - ref.float()).abs().max())
    print(f"random weights: max |hip - torch fp16 forward| = {d:.4f} on outputs of max {float(ref.float().abs().max()):.3f}")
    photo = torch.from_numpy(g.integers(0, 256, size=(1024, 1024, 3), dtype=np.uint8)).to(dev)
    tmpl = ffhq_template(512)
    face = lambda tx, ty: (tx, ty, 400.0, 400.0, 0.99, (tmpl * 0.9 + [tx, ty]).tolist())
    all_faces = [face(20.0, 30.0), face(520.0, 40.0), face(40.0, 530.0), face(510.0, 520.0)]
    for nf in (1, 4):
        fr = FaceRestorer(net, lambda rgb, nf=nf: all_faces[:nf], device=dev)
        fr.restore_u8(photo)
        net.hip(crops[:nf])
        with torch.no_grad():
            half(nchw[:nf])
        torch.cuda.synchronize()
        rows = {"net.hip": [], "torch fp16 forward": [], "restore_u8 (1024 x 1024 photo, stub detector)": []}
        for _ in range(3):                         # alternated: three rounds of each
            rows["net.hip"].append(timed(lambda: net.hip(crops[:nf]), reps))
            with torch.no_grad():
                rows["torch fp16 forward"].append(timed(lambda: half(nchw[:nf]), reps))
            rows["restore_u8 (1024 x 1024 photo, stub detector)"].append(timed(lambda: fr.restore_u8(photo), reps))
        for k, v in rows.items():
            print(f"{nf} face(s), 512 x 512 crops, {k}: median {statistics.median(m for m, _ in v):.3f} ms, min {min(m for _, m in v):.3f} ms "
                  f"({reps} calls x 3 alternated rounds)")
    walk_ms, _ = timed(lambda: net.hip(crops[:1]), reps)
    c = net._prepare(dev)
    total_us, total_bytes = 0.0, 0
    for name, m in c.items():
        if not hasattr(m, "wsq"):
            continue
        styles = torch.ones((1, m.cin), dtype=torch.float32, device=dev)
        buf = net._weights_scratch(dev, m, 1)
        gain = math.sqrt(2.0) if m.wsq is not None else 1.0
        ops.modulate_weights(m.w, m.wsq, styles, buf, gain)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            ops.modulate_weights(m.w, m.wsq, styles, buf, gain)
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1e3 / iters
        nbytes = m.cout * m.taps * m.cin * (4 + 2) + (m.cout * m.cin * 4 if m.wsq is not None else 0) + m.cin * 4
        total_us += us
        total_bytes += nbytes
        print(f"af_modulate_weights {name}: cout {m.cout} cin {m.cin} taps {m.taps}: {us:.2f} us per call, {nbytes / 1e6:.2f} MB, "
              f"{nbytes / us / 1e6:.3f} TB/s (back to back: the master weights of the small layers stay in cache)")
    print(f"af_modulate_weights, all {sum(hasattr(m, 'wsq') for m in c.values())} layers of one crop: {total_us:.1f} us of a {walk_ms * 1e3:.0f} us walk "
          f"({100 * total_us / (walk_ms * 1e3):.1f} %), {total_bytes / 1e6:.1f} MB, {total_bytes / total_us / 1e6:.3f} TB/s overall (HBM peak 8 TB/s)")


if __name__ == "__main__":
    main()
