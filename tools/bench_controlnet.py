"""Time the ControlNet path (INTEGRATION.md "ControlNet") on one GPU.

(a) Hint encoder: ControlNet.hint_features (seven af_hint_conv3x3 launches + the tuned conv3x3) on 1 and on 16 control images of 512 x 512,
    against the torch fp16 device composition of the same eight convolutions (F.conv2d + F.silu, NCHW), with the share of the roof: the
    least time the hardware could take, max(FLOP / 2.5 PFLOP/s dense fp16, bytes / 8 TB/s), over the measured time.  FLOP and bytes (each
    layer's input read once and output written once, weights once) are computed from the shapes.
(b) Denoise step: one eager U-Net epsilon-prediction at 8 rows (batch 4 with CFG) of 64 x 64 latents (512 x 512 images), SD-1.5 widths,
    synthetic weights, with and without a ControlNet set, alternating in the same run; beside it the FLOP share of ControlNet's trunk
    computed from the shapes.

Device events, median of 9 after 2 warm-up runs.  Neither figure is a gate; (a) runs once per generation.

    python tools/bench_controlnet.py [--out profiles/controlnet.txt] [--no-torch] [--no-step]

The file is written line by line, so a run that is cut short keeps what it measured."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF, BW = 2.5e15, 8.0e12
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


def hint_layers(mc):
    """(cin, cout, stride) of the eight convolutions."""
    from adaface_dev_amd.ldm.modules.diffusionmodules.controlnet import HINT_WIDTHS
    out, cin = [], 3
    for cout, s in HINT_WIDTHS:
        out.append((cin, cout, s))
        cin = cout
    return out + [(cin, mc, 1)]


def hint_cost(B, H, W, mc):
    """(FLOP, bytes) of the hint encoder on B images of H x W: useful multiply-adds; input (uint8 for the first layer) + output + weights."""
    flop = byts = 0.0
    for k, (cin, cout, s) in enumerate(hint_layers(mc)):
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        flop += 2.0 * 9 * cin * cout * B * Ho * Wo
        byts += B * H * W * cin * (1 if k == 0 else 2) + B * Ho * Wo * cout * 2 + 9 * cin * cout * 2
        H, W = Ho, Wo
    return flop, byts


def unet_flops(cfg, h, w, L):
    """Per row: (encoder + middle block, whole U-Net, the thirteen zero convolutions) multiply-add FLOP of one epsilon-prediction on h x w latents
    with L context tokens, from the shapes (convolutions, linears and the two attention products; norms and activations not counted)."""
    mc, mult, nrb, ares, ctx = cfg["model_channels"], cfg["channel_mult"], cfg["num_res_blocks"], cfg["attention_resolutions"], cfg["context_dim"]
    emb = 4 * mc

    def res(cin, cout, n):
        return 18.0 * cin * cout * n + 18.0 * cout * cout * n + (2.0 * cin * cout * n if cin != cout else 0) + 2.0 * emb * cout

    def attn(c, n):
        return 4.0 * c * c * n + (8.0 * c * c * n + 4.0 * n * n * c) + (4.0 * c * c * n + 4.0 * ctx * c * L + 4.0 * n * L * c) + 24.0 * c * c * n

    enc = 18.0 * cfg["in_channels"] * mc * h * w + 2.0 * mc * emb + 2.0 * emb * emb
    zero = 2.0 * mc * mc * h * w
    chans, ch, ds, n = [mc], mc, 1, h * w
    for level, m in enumerate(mult):
        for _ in range(nrb):
            enc += res(ch, m * mc, n) + (attn(m * mc, n) if ds in ares else 0)
            ch = m * mc
            chans.append(ch)
            zero += 2.0 * ch * ch * n
        if level != len(mult) - 1:
            n //= 4
            enc += 18.0 * ch * ch * n
            chans.append(ch)
            zero += 2.0 * ch * ch * n
            ds *= 2
    mid = 2 * res(ch, ch, n) + attn(ch, n)
    zero += 2.0 * ch * ch * n
    dec = 0.0
    for level, m in list(enumerate(mult))[::-1]:
        for i in range(nrb + 1):
            dec += res(ch + chans.pop(), m * mc, n) + (attn(m * mc, n) if ds in ares else 0)
            ch = m * mc
            if level and i == nrb:
                n *= 4
                dec += 18.0 * ch * ch * n
                ds //= 2
    dec += 18.0 * mc * cfg["out_channels"] * h * w
    return enc + mid, enc + mid + dec, zero


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "controlnet.txt"))
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition (its first convolutions search for a kernel)")
    ap.add_argument("--no-step", action="store_true", help="skip (b), the full-width denoise step")
    args = ap.parse_args()
    from adaface_dev_amd import SD15_UNET_CONFIG, _lib, rng
    from adaface_dev_amd.ldm.modules.diffusionmodules.controlnet import ControlNet
    from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    _lib.lib()
    dev = torch.device("cuda:0")
    out = open(args.out, "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    cfg = SD15_UNET_CONFIG
    mc = cfg["model_channels"]
    say(f"tools/bench_controlnet.py on {torch.cuda.get_device_name(0)}: device events, median of {REPS} after {WARM} warm-up runs; fp16, SD-1.5 widths, "
        "synthetic weights")
    say()
    with rng.skip_default_init():
        cn = ControlNet(**cfg)
    rng.load_synth_weights(cn.to(dev), seed=3, on_device=True)
    g = torch.Generator().manual_seed(0)
    say("(a) hint encoder, 512 x 512 control images -> [B0, 64, 64, 320]: ControlNet.hint_features (7 x af_hint_conv3x3 + the tuned conv3x3) against "
        "the torch fp16 composition (F.conv2d + F.silu, NCHW)")
    say(f"    roof share = max(FLOP / {ROOF / 1e15:.1f} PFLOP/s, bytes / {BW / 1e12:.0f} TB/s) / measured time; FLOP and bytes from the shapes")
    say(f"{'images':>8}{'GFLOP':>9}{'MB':>8}{'bound':>8}{'least us':>10}{'hip ms':>9}{'TFLOP/s':>9}{'of fp16 roof':>14}{'roof share':>12}{'torch ms':>10}")
    ws = [(m.weight.detach().half(), m.bias.detach().half(), m.stride[0]) for m in cn.input_hint_block if hasattr(m, "weight")]
    for B0 in (1, 16):
        img = torch.randint(0, 256, (B0, 512, 512, 3), generator=g, dtype=torch.uint8).to(dev)
        flop, byts = hint_cost(B0, 512, 512, mc)
        least = max(flop / ROOF, byts / BW)
        with torch.no_grad():
            ms = median_ms(lambda: cn.hint_features(img))
            tms = "-"
            if not args.no_torch:
                def tfn():
                    x = img.permute(0, 3, 1, 2).half() / 255
                    for k, (wt, b, s) in enumerate(ws):
                        x = F.conv2d(x, wt, b, stride=s, padding=1)
                        if k < len(ws) - 1:
                            x = F.silu(x)
                    return x
                tms = f"{median_ms(tfn):.3f}"
        say(f"{B0:>8}{flop / 1e9:>9.2f}{byts / 1e6:>8.1f}{'memory' if byts / BW > flop / ROOF else 'compute':>8}{least * 1e6:>10.1f}{ms:>9.3f}"
            f"{flop / ms / 1e9:>9.1f}{flop / ms * 1e3 / ROOF:>14.4f}{least * 1e3 / ms:>12.3f}{tms:>10}")
        del img
    say()
    enc, total, zero = unet_flops(cfg, 64, 64, 77)
    say("(b) eager denoise step, 8 rows (batch 4 with CFG) of 64 x 64 latents, 77 context tokens")
    say(f"    FLOP per row from the shapes: U-Net {total / 1e9:.1f} G; ControlNet trunk (the encoder and middle block over again) {enc / 1e9:.1f} G + thirteen "
        f"zero convolutions {zero / 1e9:.2f} G = {(enc + zero) / total:.3f} of the U-Net's")
    if not args.no_step:
        with rng.skip_default_init():
            unet = UNetModel(**cfg)
        rng.load_synth_weights(unet.to(dev).eval(), seed=1, on_device=True)
        x = torch.randn(8, 4, 64, 64, device=dev)
        t = torch.full((8,), 500, device=dev, dtype=torch.long)
        ctx = torch.randn(8, 77, cfg["context_dim"], device=dev)
        img = torch.randint(0, 256, (4, 512, 512, 3), generator=g, dtype=torch.uint8).to(dev)
        with torch.no_grad():
            hint = cn.hint_features(img)
            step = lambda: unet(x, t, ctx, extra_info={})
            rounds = []
            for _ in range(2):                                  # the two versions alternate in one run
                unet.set_control(None)
                plain = median_ms(step)
                unet.set_control(cn, hint, 1.0)
                try:
                    ctl = median_ms(step)
                finally:
                    unet.set_control(None)
                rounds.append((plain, ctl))
        for k, (plain, ctl) in enumerate(rounds):
            say(f"    round {k}: U-Net {plain:.2f} ms, U-Net + ControlNet {ctl:.2f} ms = {ctl / plain:.3f} x (FLOP: {1 + (enc + zero) / total:.3f} x)")
    out.close()


if __name__ == "__main__":
    main()
