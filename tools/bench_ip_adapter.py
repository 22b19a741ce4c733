"""Time the IP-Adapter path (INTEGRATION.md "IP-Adapter") on one GPU.

(a) Kernel: af_ip_attention_add (ops.ip_attention_add) at the four U-Net shapes of an 8-row 512 x 512 batch, (N, d) = (4096, 40), (1024, 80),
    (256, 160), (64, 160) with 8 heads, each at T = 4 and T = 16 image tokens, against the composition it replaces -- ops.attention with
    L = T into a temporary (its 64-key tile mostly padding) plus torch ``add_`` with the scale -- and against the memory roof
    2 * B * N * C * 3 bytes (q read, o read and written) / 8 TB/s.  FLOP (4 T d per query and head) / 2.5 PFLOP/s is printed beside it: the larger
    of the two is the bound.  The two arms alternate in one run; the spread is (max - min) / median of each arm's own repeats.
(b) Denoise step: one eager U-Net epsilon-prediction at 8 rows (batch 4 with CFG) of 64 x 64 latents, SD-1.5 widths, synthetic weights: plain,
    plain with the one-launch cross-attention routes switched off (what an adapter forces on attn2), and with an adapter set, alternating.
    The difference adapter - plain splits into (plain split - plain), the loss of the one-launch C = 320 block, and (adapter - plain split),
    the 16 launches; beside it the sum of the kernel's own times from (a) over the 16 layers.

Device events, median of 11 after 3 warm-up runs.  Neither figure is a gate.

    python tools/bench_ip_adapter.py [--out profiles/ip_adapter.txt] [--no-step]

The file is written line by line, so a run that is cut short keeps what it measured."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF, BW = 2.5e15, 8.0e12
REPS, WARM = 11, 3
SHAPES = ((4096, 40), (1024, 80), (256, 160), (64, 160))       # (N, d) of the four U-Net levels at 64 x 64 latents
B, HEADS = 8, 8


def times_ms(fn):
    """(median, min, max) over REPS after WARM warm-up runs, device events."""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[REPS // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ip_adapter.txt"))
    ap.add_argument("--no-step", action="store_true", help="skip (b), the full-width denoise step")
    args = ap.parse_args()
    from adaface_dev_amd import SD15_UNET_CONFIG, _lib, ops, rng
    from adaface_dev_amd.adaface.ip_adapter import IPAdapter
    from adaface_dev_amd.ldm.modules import attention as A
    from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    _lib.lib()
    dev = torch.device("cuda:0")
    out = open(args.out, "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    say(f"tools/bench_ip_adapter.py on {torch.cuda.get_device_name(0)}: device events, median of {REPS} after {WARM} warm-up runs; fp16")
    say()
    say(f"(a) af_ip_attention_add, B = {B}, {HEADS} heads, against ops.attention (L = T, into a temporary) + torch add_; the arms alternate")
    say(f"    roof = max(2 * B * N * C * 3 bytes / {BW / 1e12:.0f} TB/s, 4 T d B N heads FLOP / {ROOF / 1e15:.1f} PFLOP/s); spread = (max - min) / median of the arm's repeats")
    say(f"{'N':>6}{'d':>5}{'T':>4}{'MB':>8}{'bound':>9}{'least us':>10}{'kernel us':>11}{'spread':>8}{'roof share':>12}{'compos. us':>12}{'spread':>8}{'kernel / compos.':>18}  verdict")
    g = torch.Generator().manual_seed(0)
    kernel_us = {}
    slower = []
    for N, d in SHAPES:
        C = HEADS * d
        for T in (4, 16):
            q = torch.randn((B * N, C), generator=g).to(dev, torch.float16)
            o = torch.randn((B * N, C), generator=g).to(dev, torch.float16)
            kv = torch.randn((B, T, 2 * C), generator=g).to(dev, torch.float16)
            k, v = kv[:, :, :C], kv[:, :, C:]
            k2d = kv.reshape(B * T, 2 * C)
            vt = torch.zeros((B, C, 64), dtype=torch.float16, device=dev)           # the attention kernel's layout: V transposed, keys contiguous
            vt[:, :, :T] = v.transpose(1, 2)
            scale = 0.01                                                             # small, so that the in-place arm stays finite over the repeats

            def kern():
                ops.ip_attention_add(o, q, k, v, B=B, N=N, heads=HEADS, d=d, ip_scale=scale)

            def comp():
                tmp = ops.attention(q, k2d, vt, B=B, Nq=N, L=T, heads=HEADS, d=d, ldq=C, ldk=2 * C)
                o.add_(tmp, alpha=scale)

            rk, rc = [], []
            for _ in range(2):
                rk.append(times_ms(kern))
                rc.append(times_ms(comp))
            mk, mc_ = min(r[0] for r in rk), min(r[0] for r in rc)
            sk = max((r[2] - r[1]) / r[0] for r in rk)
            sc = max((r[2] - r[1]) / r[0] for r in rc)
            byts, flop = 2.0 * B * N * C * 3, 4.0 * T * d * B * N * HEADS
            least = max(byts / BW, flop / ROOF)
            ok = mk <= mc_ * (1 + max(sk, sc))
            if not ok:
                slower.append((N, d, T))
            kernel_us[N, d, T] = mk * 1e3
            say(f"{N:>6}{d:>5}{T:>4}{byts / 1e6:>8.1f}{'memory' if byts / BW >= flop / ROOF else 'compute':>9}{least * 1e6:>10.2f}{mk * 1e3:>11.2f}{sk:>8.2f}"
                f"{least * 1e3 / mk:>12.3f}{mc_ * 1e3:>12.2f}{sc:>8.2f}{mk / mc_:>18.3f}  {'no slower' if ok else 'SLOWER'}")
    say()
    say("    every shape: the kernel is no slower than the composition beyond the spread" if not slower else
        f"    SLOWER than the composition beyond the spread at (N, d, T) = {slower}")
    say()
    if not args.no_step:
        cfg = SD15_UNET_CONFIG
        say("(b) eager denoise step, 8 rows (batch 4 with CFG) of 64 x 64 latents, 77 context tokens, T = 4 image tokens per row")
        with rng.skip_default_init():
            unet = UNetModel(**cfg)
            ad = IPAdapter(cfg, "clip")
        rng.load_synth_weights(unet.to(dev).eval(), seed=1, on_device=True)
        rng.load_synth_weights(ad.to(dev).eval(), seed=2, on_device=True)
        x = torch.randn(8, 4, 64, 64, device=dev)
        t = torch.full((8,), 500, device=dev, dtype=torch.long)
        ctx = torch.randn(8, 77, cfg["context_dim"], device=dev)
        tok = torch.randn(4, 4, cfg["context_dim"], device=dev).to(torch.float16)
        per_level = {}
        for m in unet._cross_attn_layers():
            per_level[m.dim_head] = per_level.get(m.dim_head, 0) + 1
        with torch.no_grad():
            step = lambda: unet(x, t, ctx, extra_info={})
            rounds = []
            for _ in range(2):                                  # the three versions alternate in one run
                unet.set_ip_adapter(None)
                plain = times_ms(step)[0]
                fuse, A.FUSE_XATTN = A.FUSE_XATTN, False       # read at call time by xattn_route: every attn2 runs "split"
                try:
                    split = times_ms(step)[0]
                finally:
                    A.FUSE_XATTN = fuse
                unet.set_ip_adapter(ad, tok, tok.flip(0), 1.0)
                try:
                    ip = times_ms(step)[0]
                finally:
                    unet.set_ip_adapter(None)
                rounds.append((plain, split, ip))
        # the 16 layers: 5 at 64 x 64 (d 40), 5 at 32 x 32 (d 80), 5 at 16 x 16 and the middle block at 8 x 8 (d 160)
        n160 = per_level.get(160, 0)
        own = (per_level.get(40, 0) * kernel_us[4096, 40, 4] + per_level.get(80, 0) * kernel_us[1024, 80, 4] + (n160 - 1) * kernel_us[256, 160, 4]
               + kernel_us[64, 160, 4]) / 1e3
        say(f"    cross-attention layers by head dim: {per_level}; the kernel's own times from (a) over them sum to {own:.3f} ms")
        for i, (plain, split, ip) in enumerate(rounds):
            say(f"    round {i}: plain {plain:.2f} ms, plain with attn2 split {split:.2f} ms, with the adapter {ip:.2f} ms: + {ip - plain:.2f} ms = "
                f"{split - plain:+.2f} ms (loss of the one-launch C = 320 block) {ip - split:+.2f} ms (the 16 launches)")
    out.close()


if __name__ == "__main__":
    main()
