"""Time the Real-ESRGAN path (INTEGRATION.md "Upscaling (Real-ESRGAN)") on one GPU: af_dense_conv3x3 at the five body shapes and the tail
shapes of a 512 x 512 x4 run, and the whole RRDBNet.hip at 512 x 512 with the x4 and the x2 network (23 blocks, synthetic weights), each
against the torch device composition in fp16 (F.conv2d, torch.cat, F.leaky_relu, F.interpolate).  Device events, median of 9 after 2 warm-up
runs.  FLOP/s are quoted against the 2.5 PFLOP/s dense fp16 roof.

    python tools/bench_esrgan.py [--out profiles/esrgan.txt] [--no-torch]

The file is written line by line, so a run that is cut short keeps what it measured."""
import argparse
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF = 2.5e15
REPS, WARM = 9, 2


def median_ms(fn):
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
    return sorted(ts)[REPS // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "esrgan.txt"))
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition (its first convolutions search for a kernel)")
    args = ap.parse_args()
    from adaface_dev_amd import _lib, ops
    from adaface_dev_amd.adaface.esrgan import RRDBNet
    _lib.lib()
    dev = torch.device("cuda:0")
    out = open(args.out, "w")

    def say(line=""):
        print(line)
        out.write(line + "\n")
        out.flush()

    say(f"tools/bench_esrgan.py on {torch.cuda.get_device_name(0)}: device events, median of {REPS} after {WARM} warm-up runs; fp16, batch 1")
    say(f"FLOP/s against the {ROOF / 1e15:.1f} PFLOP/s dense fp16 roof; 'torch' is the fp16 device composition (F.conv2d on the materialised torch.cat, "
        "F.leaky_relu, F.interpolate)")
    say()
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    # (name, H = W of the input grid, cin, cout, upsample, residual, uint8)
    shapes = [("rdb conv1", 512, 64, 32, 0, 0, 0), ("rdb conv2", 512, 96, 32, 0, 0, 0), ("rdb conv3", 512, 128, 32, 0, 0, 0),
              ("rdb conv4", 512, 160, 32, 0, 0, 0), ("rdb conv5 + residual", 512, 192, 64, 0, 1, 0), ("conv_up1 (nearest x2 fused)", 512, 64, 64, 1, 0, 0),
              ("conv_up2 (nearest x2 fused)", 1024, 64, 64, 1, 0, 0), ("conv_hr", 2048, 64, 64, 0, 0, 0), ("conv_last -> uint8", 2048, 64, 3, 0, 0, 1)]
    say("af_dense_conv3x3, one launch")
    say(f"{'shape':<30}{'grid':>11}{'cin':>5}{'cout':>5}{'GFLOP':>9}{'hip ms':>9}{'TFLOP/s':>9}{'of roof':>9}{'torch ms':>10}")
    hip_ms = {}
    for name, S, cin, cout, up, res, u8 in shapes:
        So = S * (2 if up else 1)
        ld = 192 if S == 512 else 64                    # the body and conv_up1 read a dense-block buffer, the tail a 64-channel one
        buf = torch.randn((1, S, S, ld), dtype=torch.float16, device=dev) * 0.5
        w4 = (torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)).half().to(dev)
        wt, bias = ops.dense_conv3x3_weight(w4), torch.zeros(cout, device=dev)
        flop = 2.0 * 9 * cin * cout * So * So
        if u8:
            fn = lambda: ops.dense_conv3x3_u8(buf, cin, wt, bias, cout)
        elif res:
            dst = torch.empty((1, So, So, 192), dtype=torch.float16, device=dev)      # conv5 writes channels [0, 64) of the next buffer
            fn = lambda: ops.dense_conv3x3(buf, cin, wt, bias, dst, 0, cout, r1=buf, alpha=0.2)
        elif up or cout == 64:
            dst = torch.empty((1, So, So, 64), dtype=torch.float16, device=dev)
            fn = lambda: ops.dense_conv3x3(buf, cin, wt, bias, dst, 0, cout, slope=0.2, upsample=bool(up))
        else:
            fn = lambda: ops.dense_conv3x3(buf, cin, wt, bias, buf, cin, cout, slope=0.2)
        ms = median_ms(fn)
        hip_ms[name] = ms
        tms = "-"
        if not args.no_torch:
            pieces = [buf[..., :64].permute(0, 3, 1, 2).contiguous()] + [buf[..., c:c + 32].permute(0, 3, 1, 2).contiguous() for c in range(64, cin, 32)]
            b16 = bias.half()

            def tfn():
                x = torch.cat(pieces, 1) if len(pieces) > 1 else pieces[0]
                if up:
                    x = F.interpolate(x, scale_factor=2, mode="nearest")
                y = F.conv2d(x, w4, b16, padding=1)
                if res:
                    return y * 0.2 + pieces[0]
                if u8:
                    return (y.clamp(0, 1) * 255).round().to(torch.uint8)
                return F.leaky_relu(y, 0.2)

            tms = f"{median_ms(tfn):.3f}"
        say(f"{name:<30}{So:>6}^2   {cin:>5}{cout:>5}{flop / 1e9:>9.1f}{ms:>9.3f}{flop / ms / 1e9:>9.1f}{flop / ms * 1e3 / ROOF:>9.3f}{tms:>10}")
        del buf
    say()
    say("RRDBNet.hip, 23 blocks, one 512 x 512 uint8 image in, uint8 out (351 launches of af_dense_conv3x3 + 1 of af_u8_unshuffle_f16)")
    img = torch.randint(0, 256, (1, 512, 512, 3), generator=g, dtype=torch.uint8).to(dev)
    for scale in (4, 2):
        net = RRDBNet(scale=scale, num_block=23).eval()
        Hc = 512 // net.unshuffle
        body = 23 * 3 * (32 * (64 + 96 + 128 + 160) + 64 * 192) + 64 * 64 + 64 * net.hip_cpad      # sum of cin * cout on the H/r grid (conv_first with its zero-padded input)
        flop = 2.0 * 9 * (Hc * Hc * body + 4 * Hc * Hc * 64 * 64 + 16 * Hc * Hc * (64 * 64 * 2 + 64 * 3))
        net.to(dev)
        ms = median_ms(lambda: net.hip(img))
        tms = "-"
        if not args.no_torch:
            net.half()
            x = (img.permute(0, 3, 1, 2).half() / 255).contiguous()
            with torch.no_grad():
                tms = f"{median_ms(lambda: net(x)):.2f}"
        say(f"x{scale}: {flop / 1e12:.2f} TFLOP issued, hip {ms:.2f} ms = {flop / ms / 1e9:.0f} TFLOP/s ({flop / ms * 1e3 / ROOF:.3f} of roof), torch {tms} ms")
        del net
    out.close()


if __name__ == "__main__":
    main()
