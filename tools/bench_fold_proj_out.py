"""ff.net[2] + proj_out at the denoise step's three C = 640 / 1280 shapes: the two GEMMs (K = 4C, then K = C with the block's input as residual) against
the folded K = 5C launch over [g ; x2] (ops.pack_ff_proj_out), each with the table's configuration, as a hipGraph of 20 calls over 10 different
weight sets (so the weights are not L2-hot), replays interleaved, median of 9.   python tools/bench_fold_proj_out.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from adaface_dev_amd import ops


def main():
    dev = torch.device("cuda:0")
    print("# us per feed-forward tail (second projection + proj_out), 20 per graph, interleaved replays, median of 9")
    for (M, C, rpb) in [(8192, 640, 1024), (2048, 1280, 256), (512, 1280, 64)]:
        g, x2, x_in = (torch.randn(M, 4 * C, device=dev).half(), torch.randn(M, C, device=dev).half(), torch.randn(M, C, device=dev).half())
        sets = []
        for _ in range(10):
            w2, b2, wp, bp = torch.randn(C, 4 * C) * (4 * C) ** -0.5, torch.randn(C) * 0.05, torch.randn(C, C) * C ** -0.5, torch.randn(C) * 0.05
            sets.append((ops.pack_matrix(w2, b2, dev), ops.pack_matrix(wp, bp, dev), ops.pack_ff_proj_out(w2, b2, wp, bp, dev)))

        def pair(s):
            return ops.gemm(ops.gemm(g, s[0], residual=x2), s[1], residual=x_in, rows_per_batch=rpb, gn_cpg=C // 32)

        def fold(s):
            return ops.gemm(g, s[2], a2=x2, residual=x_in, rows_per_batch=rpb, gn_cpg=C // 32)

        def graph_of(fn):
            for s in sets[:2]:
                fn(s)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for s in sets + sets:
                    fn(s)
            return gr
        variants = [("two launches", graph_of(pair)), ("folded", graph_of(fold))]
        times = {n: [] for n, _ in variants}
        for _ in range(9):
            for n, gr in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                gr.replay()
                e1.record()
                torch.cuda.synchronize()
                times[n].append(e0.elapsed_time(e1) * 50.0)
        cfg = [ops.tune_table().get(f"1,{M},{C},{K},0,0,0,0", (0, 1)) for K in (4 * C, C, 5 * C)]
        line = f"  M {M:5d} C {C:4d}  table {cfg[0]} + {cfg[1]} vs {cfg[2]}"
        for n, _ in variants:
            t = sorted(times[n])
            line += f" | {n} {t[4]:6.1f} us [min {t[0]:.1f} max {t[-1]:.1f}]"
        print(line, flush=True)


if __name__ == "__main__":
    main()
