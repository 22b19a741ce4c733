#!/usr/bin/env python
"""Face IDs from images at full size (seeded random weights): one `FaceIDExtractor.extract` of 4 photos of 512 x 512 with iresnet100 (a
stub detector with fixed landmarks: the detector network is the caller's), the crop kernel alone, and the launches of one forward.
After one warm-up (weight packing) `extract` is timed `reps` times, host wall clock closed by a device synchronise, image upload
included; the crop kernel by device events over `iters` back-to-back calls, repeated 5 times; launches are counted by the library's
own per-family profile (`ops.prof_read`).
                              python tools/e2e_face_id.py [reps] [iters]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

FAMILIES = ("gemm", "attn", "gnorm", "lnorm", "elem", "xattn")
KPS = [[182.0, 210.0], [330.0, 205.0], [258.0, 290.0], [195.0, 372.0], [322.0, 368.0]]


def main():
    from adaface_dev_amd import ops, rng
    from adaface_dev_amd.adaface.face_align import FaceIDExtractor, estimate_similarity
    from adaface_dev_amd.adaface.iresnet import iresnet100
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    dev = torch.device("cuda:0")
    with rng.skip_default_init():
        net = iresnet100().eval().to(dev)
    rng.load_synth_weights(net, seed=0, on_device=True)
    with torch.no_grad():
        for blk in net.blocks():
            blk.bn3.weight.mul_(0.2)               # random weights: keeps the 49-block residual sum inside fp16 (tests/test_hip_face_id.py)
    g = np.random.default_rng(0)
    images = [g.integers(0, 256, size=(512, 512, 3), dtype=np.uint8) for _ in range(4)]
    ex = FaceIDExtractor(net, lambda img: [(150.0, 150.0, 220.0, 280.0, 0.99, KPS)])
    _, ids = ex.extract(images)
    torch.cuda.synchronize()
    assert tuple(ids.shape) == (4, 512) and bool(torch.isfinite(ids).all())
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        ex.extract(images)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    print(f"extract, 4 images of 512 x 512, iresnet100, {reps} reps: median {statistics.median(times) * 1e3:.2f} ms min {min(times) * 1e3:.2f} ms")

    crops = torch.cat([ops.face_align_crop(torch.from_numpy(im).to(dev), torch.from_numpy(estimate_similarity(KPS)[1].astype(np.float32))[None].to(dev))
                       for im in images])
    ops.prof_reset()
    ops.prof_enable(True)
    net.forward_nhwc(crops)
    torch.cuda.synchronize()
    ops.prof_enable(False)
    counts = {name: ops.prof_read(i) for i, name in enumerate(FAMILIES)}
    total = sum(n for n, _ in counts.values())
    print(f"one forward, batch 4: {total} launches (" + ", ".join(f"{k} {n} / {ms:.3f} ms" for k, (n, ms) in counts.items() if n) + ")")

    img = torch.from_numpy(images[0]).to(dev)
    for nf in (1, 4):
        inv = torch.from_numpy(estimate_similarity(KPS)[1].astype(np.float32))[None].repeat(nf, 1, 1).contiguous().to(dev)
        us = []
        for _ in range(5):
            ops.face_align_crop(img, inv)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                ops.face_align_crop(img, inv)
            b.record()
            torch.cuda.synchronize()
            us.append(a.elapsed_time(b) * 1e3 / iters)
        print(f"af_face_align_crop alone, 512 x 512 image, F = {nf} ({nf * 112 * 112 * 16 / 1e3:.0f} KB written): median "
              f"{statistics.median(us):.2f} us min {min(us):.2f} us per call ({iters} back-to-back calls, allocation of the output included)")


if __name__ == "__main__":
    main()
