"""Nearest x2 + 3x3 at the denoise step's two Upsample shapes: the nine-tap gather on tile 14 (today's launch) against the four-phase form
(ops.conv3x3_up2), each as a hipGraph of 20 calls over 10 different weight tensors (so the weights are not L2-hot), replays interleaved,
median of 9.   python tools/bench_up2.py [B]
With a second argument `8x8`: the 8 x 8 -> 16 x 16 level instead (1280 -> 1280), the nine-tap launch as the table has it against the phase form on every
whole-line tile / split count the library takes there (af_gemm_halo_variant 5).   python tools/bench_up2.py 8 8x8"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from adaface_dev_amd import ops


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    dev = torch.device("cuda:0")
    print(f"# batch {B}: us per launch (algorithmic nine-tap TFLOP/s), 20 launches per graph, interleaved replays, median of 9")
    small = len(sys.argv) > 2 and sys.argv[2] == "8x8"
    for (HW, c) in ([(8, 1280)] if small else [(16, 1280), (32, 640)]):
        x = torch.randn(B, HW, HW, c, device=dev).half()
        ws = [torch.randn(c, c, 3, 3) * (9 * c) ** -0.5 for _ in range(10)]
        p9 = [ops.pack_conv3x3(w, torch.zeros(c), dev) for w in ws]
        p4 = [ops.pack_conv3x3_up2(w, torch.zeros(c), dev) for w in ws]
        flops = 2.0 * B * 4 * HW * HW * c * 9 * c

        def graph_of(fn, packs):
            for pw in packs[:2]:
                fn(x, pw)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for pw in packs + packs:
                    fn(x, pw)
            return g
        if small:
            variants = [("nine-tap table", graph_of(lambda a, pw: ops.conv3x3(a, pw, upsample=True), p9))]
            for tile in (7, 8, 11, 12, 13):
                for sp in (2, 3, 4, 6, 8):
                    if ops.conv_up2_eligible(ops.conv_up2_desc(B, HW, HW, c, c, tile=tile, splits=sp)):
                        variants.append((f"phase t{tile}x{sp}", graph_of(lambda a, pw, tile=tile, sp=sp: ops.conv3x3_up2(a, pw, tile=tile, splits=sp), p4)))
        else:
            variants = [("nine-tap t14", graph_of(lambda a, pw: ops.conv3x3(a, pw, upsample=True, tile=14, splits=1), p9)),
                        ("phase t14", graph_of(lambda a, pw: ops.conv3x3_up2(a, pw), p4))]
        times = {n: [] for n, _ in variants}
        for _ in range(9):
            for n, g in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.replay()
                e1.record()
                torch.cuda.synchronize()
                times[n].append(e0.elapsed_time(e1) * 50.0)
        line = f"  {HW}x{HW} -> {2 * HW}x{2 * HW} {c:4d}->{c:4d} "
        for n, _ in variants:
            t = sorted(times[n])
            line += ("\n    " if small else " | ") + f"{n} {t[4]:6.1f} us ({flops / t[4] * 1e-6:4.0f}) [min {t[0]:.1f} max {t[-1]:.1f}]"
        print(line, flush=True)


if __name__ == "__main__":
    main()
