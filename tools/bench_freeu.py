"""Time FreeU (INTEGRATION.md "FreeU") on one GPU.

(a) Kernels: the af_freeu_stats + af_freeu_apply pair (ops.freeu, version 2) at the ten (h, skip) shapes FreeU touches in an 8-row 512 x 512
    batch of SD-1.5 (output blocks 0 .. 6 with (b1, s1) = (1.5, 0.9), 7 .. 9 with (b2, s2) = (1.6, 0.2)), against the torch composition it
    replaces, written here: NHWC fp16 -> NCHW fp32, the channel mean with its per-sample min / max and the scaled slice write, fftn / fftshift /
    mask multiply / ifftshift / ifftn / .real, and the conversions back.  The pair is timed as a hipGraph of 10 calls (replayed, device events
    around the replay) and eagerly (device events around 10 back-to-back calls); the torch composition eagerly only (its FFT plans are not
    captured here), so compare eager with eager.  The pair writes into separate outputs here so that ten calls see the same data; in the U-Net it
    runs in place, with the same traffic.  Bytes: what the algorithm must move -- stats reads h and skip once, apply reads and writes half of h
    and all of skip: (2 C + 3 Cs) B H W 2 bytes -- against the 8 TB/s HBM roof.
(b) Denoise step: one eager U-Net epsilon-prediction at 8 rows (batch 4 with CFG) of 64 x 64 latents, SD-1.5 widths, synthetic weights, with
    FreeU unset and set, alternating, and the launches counted through ops._launch in both states.

Median of REPS after WARM warm-up runs; spread = (max - min) / median of an arm's repeats.  No figure is a gate.

    python tools/bench_freeu.py [--out profiles/freeu.txt] [--no-step]

The file is written line by line, so a run that is cut short keeps what it measured."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM, ITERS = 9, 2, 10
B = 8
#         block(s)  H   W   C     Cs    b    s
SHAPES = (("0-2", 8, 8, 1280, 1280, 1.5, 0.9), ("3-4", 16, 16, 1280, 1280, 1.5, 0.9), ("5", 16, 16, 1280, 640, 1.5, 0.9),
          ("6", 32, 32, 1280, 640, 1.5, 0.9), ("7", 32, 32, 640, 640, 1.6, 0.2), ("8", 32, 32, 640, 320, 1.6, 0.2),
          ("9", 64, 64, 640, 320, 1.6, 0.2))
HBM_TBS = 8.0


def median_us(run, per):
    """(median, min, max) in us per call: ``run`` enqueues ``per`` calls; device events around it."""
    for _ in range(WARM):
        run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / per)
    ts.sort()
    return ts[REPS // 2], ts[0], ts[-1]


def torch_freeu(h, skip, b, s):
    """The composition FreeU costs when written with torch on the device (the authors' code on this project's layout)."""
    hn = h.permute(0, 3, 1, 2).float()
    kn = skip.permute(0, 3, 1, 2).float()
    Bn, C = hn.shape[:2]
    m = hn.mean(1, keepdim=True)
    lo = m.reshape(Bn, -1).min(-1)[0].reshape(Bn, 1, 1, 1)
    hi = m.reshape(Bn, -1).max(-1)[0].reshape(Bn, 1, 1, 1)
    mh = (m - lo) / (hi - lo)
    hn[:, :C // 2] = hn[:, :C // 2] * ((b - 1.0) * mh + 1.0)
    f = torch.fft.fftshift(torch.fft.fftn(kn, dim=(-2, -1)), dim=(-2, -1))
    H, W = f.shape[-2:]
    mask = torch.ones((1, 1, H, W), device=f.device)
    mask[..., H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = s
    kn = torch.fft.ifftn(torch.fft.ifftshift(f * mask, dim=(-2, -1)), dim=(-2, -1)).real
    return hn.permute(0, 2, 3, 1).to(torch.float16).contiguous(), kn.permute(0, 2, 3, 1).to(torch.float16).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freeu.txt"))
    ap.add_argument("--no-step", action="store_true", help="skip (b), the full-width denoise step")
    args = ap.parse_args()
    from adaface_dev_amd import SD15_UNET_CONFIG, _lib, ops, rng
    from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    _lib.lib()
    dev = torch.device("cuda:0")
    out = open(args.out, "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    say(f"tools/bench_freeu.py on {torch.cuda.get_device_name(0)}: median of {REPS} after {WARM} warm-up runs, {ITERS} calls per timed run; fp16, B = {B}, version 2")
    say()
    say("(a) af_freeu_stats + af_freeu_apply (ops.freeu) against the torch composition (layout conversions, mean / min / max / slice write, torch.fft)")
    say(f"{'blocks':>7}{'H x W':>9}{'C':>6}{'Cs':>6}{'MB':>8}{'graph us':>10}{'spread':>8}{'of roof':>9}{'eager us':>10}{'spread':>8}{'torch us':>10}{'spread':>8}"
        f"{'eager / torch':>15}  verdict")
    g = torch.Generator().manual_seed(0)
    slower, total_graph, total_torch, n_blocks = [], 0.0, 0.0, {"0-2": 3, "3-4": 2}
    for name, H, W, C, Cs, b, s in SHAPES:
        h = (torch.randn((B, H, W, C), generator=g) + 2.0).to(dev, torch.float16)
        skip = (torch.randn((B, H, W, Cs), generator=g) + 2.0).to(dev, torch.float16)
        oh, ok = h.clone(), skip.clone()

        def pair_kernels():                                  # the two launches alone (ops.freeu's out-of-place form also copies the upper half of h)
            ws = ops.freeu_stats(h, skip, b, s, 2)
            ops._launch("af_freeu_apply", h.data_ptr(), skip.data_ptr(), ws.data_ptr(), ws.numel(), oh.data_ptr(), ok.data_ptr(), B, H, W, C, Cs, b, s, 2)

        for _ in range(3):
            pair_kernels()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(ITERS):
                pair_kernels()
        tg = median_us(gr.replay, ITERS)
        te = median_us(lambda: [pair_kernels() for _ in range(ITERS)], ITERS)
        tt = median_us(lambda: [torch_freeu(h, skip, b, s) for _ in range(ITERS)], ITERS)
        del gr
        mb = (2 * C + 3 * Cs) * B * H * W * 2 / 1e6
        roof_us = mb / (HBM_TBS * 1e6) * 1e6
        ok_ = te[0] <= tt[0] * (1 + max((te[2] - te[1]) / te[0], (tt[2] - tt[1]) / tt[0]))
        if not ok_:
            slower.append(name)
        total_graph += tg[0] * n_blocks.get(name, 1)
        total_torch += tt[0] * n_blocks.get(name, 1)
        say(f"{name:>7}{f'{H} x {W}':>9}{C:>6}{Cs:>6}{mb:>8.1f}{tg[0]:>10.2f}{(tg[2] - tg[1]) / tg[0]:>8.2f}{roof_us / tg[0]:>9.3f}{te[0]:>10.2f}"
            f"{(te[2] - te[1]) / te[0]:>8.2f}{tt[0]:>10.2f}{(tt[2] - tt[1]) / tt[0]:>8.2f}{te[0] / tt[0]:>15.3f}  {'no slower' if ok_ else 'SLOWER'}")
    say()
    say(f"    all ten blocks of one U-Net call: the pair (graph) {total_graph:.0f} us, the torch composition (eager) {total_torch:.0f} us")
    say("    every shape: the pair is no slower than the torch composition beyond the spread" if not slower else
        f"    SLOWER than the torch composition beyond the spread at blocks {slower}")
    say()
    if not args.no_step:
        cfg = SD15_UNET_CONFIG
        say("(b) eager denoise step, 8 rows (batch 4 with CFG) of 64 x 64 latents, 77 context tokens; FreeU = (b1, b2, s1, s2) = (1.5, 1.6, 0.9, 0.2), version 2")
        with rng.skip_default_init():
            unet = UNetModel(**cfg)
        rng.load_synth_weights(unet.to(dev).eval(), seed=1, on_device=True)
        x = torch.randn(8, 4, 64, 64, device=dev)
        t = torch.full((8,), 500, device=dev, dtype=torch.long)
        ctx = torch.randn(8, 77, cfg["context_dim"], device=dev)
        real, names = ops._launch, []
        with torch.no_grad():
            step = lambda: unet(x, t, ctx, extra_info={})
            step()
            counts = []
            for on in (False, True):
                unet.set_freeu(1.5, 1.6, 0.9, 0.2) if on else unet.set_freeu(None)
                ops._launch = lambda name, *a, **k: names.append(name) or real(name, *a, **k)
                try:
                    names.clear()
                    step()
                    counts.append((len(names), sum("freeu" in n for n in names)))
                finally:
                    ops._launch = real
            say(f"    launches through ops._launch in one step: FreeU unset {counts[0][0]} (af_freeu_*: {counts[0][1]}), set {counts[1][0]} (af_freeu_*: {counts[1][1]})")
            for i in range(2):                                  # the two states alternate in one run
                unet.set_freeu(None)
                off = median_us(step, 1)
                unet.set_freeu(1.5, 1.6, 0.9, 0.2)
                on = median_us(step, 1)
                unet.set_freeu(None)
                say(f"    round {i}: FreeU unset {off[0] / 1e3:.2f} ms (spread {(off[2] - off[1]) / off[0]:.2f}), set {on[0] / 1e3:.2f} ms "
                    f"(spread {(on[2] - on[1]) / on[0]:.2f}): + {(on[0] - off[0]) / 1e3:.2f} ms")
    out.close()


if __name__ == "__main__":
    main()
