"""The three launches of "repaint the faces of a photo" (csrc/af_repaint.hip) at a user's size -- a 3000 x 2000 photo, a 900 px region, work
size 512 x 512, B = 4 outputs -- against the composition of torch device ops doing the same job (F.interpolate(antialias=True), the blend and
the uint8 conversion).  Device events around 20 calls, the two forms interleaved, median of 9 rounds after a warm-up; bytes are the
algorithm's (computed from the shapes), so GB/s is achieved traffic, not a counter.   python tools/bench_face_repaint.py [B]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from adaface_dev_amd import ops

H, W, RECT, WORK, THR, FEATHER = 2000, 3000, (1050, 550, 900, 900), (512, 512), 1.0 / 255.0, 0.25
CALLS, ROUNDS = 20, 9


def torch_alpha(ell, feather):
    ys = torch.arange(H, device=ell.device, dtype=torch.float32)[:, None] + 0.5
    xs = torch.arange(W, device=ell.device, dtype=torch.float32)[None, :] + 0.5
    a = torch.zeros(H, W, device=ell.device)
    for cx, cy, rx, ry in ell.tolist():
        t = ((1 - torch.sqrt(((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2)) / feather).clamp(0, 1)
        a = torch.maximum(a, t * t * (3 - 2 * t))
    return a


def torch_crop(photo, alpha):
    x0, y0, cw, ch = RECT
    kw = dict(size=WORK, mode="bilinear", antialias=True, align_corners=False)
    img = F.interpolate(photo[y0:y0 + ch, x0:x0 + cw].permute(2, 0, 1)[None].float(), **kw)
    img = img.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    a = F.interpolate(alpha[None, None, y0:y0 + ch, x0:x0 + cw], **kw)
    return img, (F.max_pool2d(a, 8) >= THR).float()


def torch_paste(dec, photo, alpha):
    x0, y0, cw, ch = RECT
    d = F.interpolate(dec, size=(ch, cw), mode="bilinear", antialias=True, align_corners=False)
    g = (255 * (d / 2 + 0.5).clamp(0, 1)).permute(0, 2, 3, 1)
    a = alpha[y0:y0 + ch, x0:x0 + cw, None]
    out = photo[None].repeat(dec.shape[0], 1, 1, 1)
    out[:, y0:y0 + ch, x0:x0 + cw] = (a * g + (1 - a) * photo[y0:y0 + ch, x0:x0 + cw].float()).round().to(torch.uint8)
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / CALLS


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    photo = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    dec = (torch.rand((B, 3) + WORK, generator=g) * 2.4 - 1.2).to(dev)
    x0, y0, cw, ch = RECT
    ell = torch.tensor([[x0 + 0.35 * cw, y0 + 0.5 * ch, 0.17 * cw, 0.22 * ch], [x0 + 0.68 * cw, y0 + 0.45 * ch, 0.15 * cw, 0.2 * ch]],
                       dtype=torch.float32, device=dev)
    alpha = ops.face_alpha_mask(ell, (H, W), FEATHER)
    cells = (WORK[0] // 8) * (WORK[1] // 8)
    inside = int((alpha[y0:y0 + ch, x0:x0 + cw] > 0).sum())
    jobs = [
        ("af_face_alpha_mask", H * W * 4, lambda: ops.face_alpha_mask(ell, (H, W), FEATHER), lambda: torch_alpha(ell, FEATHER)),
        ("af_crop_resize_u8", ch * cw * 7 + WORK[0] * WORK[1] * 3 + cells * 4, lambda: ops.crop_resize_u8(photo, alpha, RECT, WORK, THR),
         lambda: torch_crop(photo, alpha)),
        ("af_paste_back_u8", H * W * 3 * (1 + B) + ch * cw * 4 + B * 3 * WORK[0] * WORK[1] * 4, lambda: ops.paste_back_u8(dec, photo, alpha, RECT),
         lambda: torch_paste(dec, photo, alpha)),
    ]
    print(f"# {W} x {H} photo, region {RECT}, work size {WORK[1]} x {WORK[0]}, B = {B}, {inside} pixels with alpha > 0; us per call, "
          f"{CALLS} calls per timing, interleaved, median of {ROUNDS} [min max]; GB/s = algorithmic bytes / median")
    da = (alpha - torch_alpha(ell, FEATHER)).abs().max().item()
    (ik, mk), (it, mt) = ops.crop_resize_u8(photo, alpha, RECT, WORK, THR), torch_crop(photo, alpha)
    dp = (ops.paste_back_u8(dec, photo, alpha, RECT).int() - torch_paste(dec, photo, alpha).int()).abs().max().item()
    print(f"# kernel vs torch composition: alpha max diff {da:.2e}; crop image max diff {(ik.int() - it.int()).abs().max().item()} level(s), "
          f"latent mask cells differing {int((mk != mt).sum())}; paste-back max diff {dp} level(s)")
    print(f"# {'launch':<20} {'MB moved':>9} | {'HIP kernel us':>14} {'GB/s':>7} {'[min max]':>16} | {'torch ops us':>13} {'[min max]':>18}")
    for name, nbytes, hip, ref in jobs:
        for _ in range(3):
            hip(), ref()
        torch.cuda.synchronize()
        th, tr = [], []
        for _ in range(ROUNDS):
            th.append(timed(hip))
            tr.append(timed(ref))
        th.sort(), tr.sort()
        mh, mr = th[ROUNDS // 2], tr[ROUNDS // 2]
        print(f"  {name:<20} {nbytes / 1e6:9.1f} | {mh:14.1f} {nbytes / mh * 1e-3:7.0f} {f'[{th[0]:.1f} {th[-1]:.1f}]':>16} | {mr:13.1f} "
              f"{f'[{tr[0]:.1f} {tr[-1]:.1f}]':>18}", flush=True)


if __name__ == "__main__":
    main()
