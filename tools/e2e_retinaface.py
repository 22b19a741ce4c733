#!/usr/bin/env python
"""RetinaFace-R50 at full size (seeded random weights): `RetinaFaceDetector.detect_batch` at batch 1 and 8, 512 x 512 and 640 x 640, and the
launches of one call.  After one warm-up (weight packing) a call is timed `reps` times, host wall clock closed by the call's own
device-to-host copy, images already on the device; launches and device time per family are the library's own profile (`ops.prof_read`).
The confidence threshold is 0.99: random weights pass arbitrary anchors, and more than 1024 of them per image is an error by design.
                              python tools/e2e_retinaface.py [reps]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

FAMILIES = ("gemm", "attn", "gnorm", "lnorm", "elem", "xattn")


def main():
    from adaface_dev_amd import ops, rng
    from adaface_dev_amd.adaface.retinaface import RetinaFace, RetinaFaceDetector
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    dev = torch.device("cuda:0")
    with rng.skip_default_init():
        net = RetinaFace().to(dev)
    rng.load_synth_weights(net, seed=0, on_device=True)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_var.fill_(1.0)
    det = RetinaFaceDetector(net, conf_threshold=0.99, preprocess="ternaus")
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    for side in (512, 640):
        for B in (1, 8):
            images = torch.randint(0, 256, (B, side, side, 3), dtype=torch.uint8, device=dev, generator=g)
            table, counts = det.detect_batch(images)
            assert bool(torch.isfinite(table).all())
            times = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t = time.perf_counter()
                det.detect_batch(images)
                times.append(time.perf_counter() - t)
            ops.prof_reset()
            ops.prof_enable(True)
            det.detect_batch(images)
            ops.prof_enable(False)
            fam = {name: ops.prof_read(i) for i, name in enumerate(FAMILIES)}
            print(f"detect_batch B = {B}, {side} x {side}, {reps} reps: median {statistics.median(times) * 1e3:.2f} ms min {min(times) * 1e3:.2f} ms; "
                  f"passing per image {counts[:, 1].tolist()}; launches " + ", ".join(f"{k} {n} / {ms:.3f} ms" for k, (n, ms) in fam.items() if n))


if __name__ == "__main__":
    main()
