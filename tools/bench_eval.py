"""The image-scoring encoders at their real sizes (evaluation/vit.py), sixteen 512 x 512 uint8 images:
  1. af_vit_patch_rows for the ViT-B/32, ViT-L/14 and DINO ViT-S/16 geometry against the torch composition it replaces (F.interpolate
     antialias in fp32, crop, normalise, unfold, cast to fp16): us per call, algorithmic bytes (images read once + rows written once),
     GB/s and the share of the 8 TB/s HBM roof, and the largest difference between the two forms;
  2. images / s of each whole encoder at batch 16 against the same module run as a torch fp16 composition (F.interpolate front,
     F.layer_norm, F.linear, F.scaled_dot_product_attention on the same weights).
Device events around CALLS calls, the two forms interleaved, median of ROUNDS rounds after a warm-up.  Seeded random weights: a checkpoint
changes no shape.   python tools/bench_eval.py [batch]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from adaface_dev_amd import ops
from adaface_dev_amd.evaluation import vit

HBM_PEAK = 8.0e12
SIDE, ROUNDS = 512, 9


def torch_rows(img, c, kcols):
    """The composition af_vit_patch_rows replaces, on device tensors."""
    Hr, Wr, top, left = ops.vit_resize_geometry(img.shape[1], img.shape[2], c.keep_aspect, c.image_size, c.image_size)
    x = F.interpolate(img.permute(0, 3, 1, 2).float(), size=(Hr, Wr), mode=c.filter, antialias=True, align_corners=False)
    x = x[:, :, top:top + c.image_size, left:left + c.image_size]
    mean = torch.tensor(c.mean, device=img.device).view(1, 3, 1, 1) * 255.0
    std = torch.tensor(c.std, device=img.device).view(1, 3, 1, 1) * 255.0
    u = F.unfold((x - mean) / std, c.patch_size, stride=c.patch_size).transpose(1, 2).reshape(-1, 3 * c.patch_size ** 2)
    return F.pad(u, (0, kcols - u.shape[1])).half()


def torch_encoder(model, img):
    """The whole tower as a torch fp16 composition on the module's own weights."""
    c = model.config
    E, T, B = c.hidden_size, model.num_patches + 1, img.shape[0]
    sd = {k: v.half() for k, v in model.state_dict().items()}
    rows = torch_rows(img, c, 3 * c.patch_size ** 2)
    x = F.linear(rows, sd["patch_embedding.weight"].reshape(E, -1), sd.get("patch_embedding.bias")).reshape(B, T - 1, E)
    h = torch.cat([sd["class_embedding"].expand(B, 1, E), x], dim=1) + sd["position_embedding"]
    ln = lambda t, n: F.layer_norm(t, (E,), sd[n + ".weight"], sd[n + ".bias"], c.layer_norm_eps)
    if c.pre_layernorm:
        h = ln(h, "pre_layrnorm")
    H = c.num_attention_heads
    for i in range(c.num_hidden_layers):
        p = f"layers.{i}."
        y = ln(h, p + "layer_norm1")
        q, k, v = (F.linear(y, sd[p + f"self_attn.{n}_proj.weight"], sd[p + f"self_attn.{n}_proj.bias"]).reshape(B, T, H, E // H).transpose(1, 2) for n in "qkv")
        o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, T, E)
        h = h + F.linear(o, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"])
        y = F.linear(ln(h, p + "layer_norm2"), sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])
        y = y * torch.sigmoid(1.702 * y) if c.hidden_act == "quick_gelu" else F.gelu(y)
        h = h + F.linear(y, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
    if c.pool == "ln_cls":
        return ln(h, "post_layernorm")[:, 0]
    return F.linear(ln(h[:, 0], "post_layernorm"), sd["visual_projection.weight"])


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / calls


def compare(hip, ref, calls):
    for _ in range(3):
        hip(), ref()
    torch.cuda.synchronize()
    th, tr = [], []
    for _ in range(ROUNDS):
        th.append(timed(hip, calls))
        tr.append(timed(ref, calls))
    th.sort(), tr.sort()
    return th, tr


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (B, SIDE, SIDE, 3), dtype=torch.uint8, generator=g).to(dev)
    models = {}
    for name, cfg in (("CLIP ViT-B/32", vit.clip_vision_config("ViT-B/32")), ("CLIP ViT-L/14", vit.clip_vision_config("ViT-L/14")),
                      ("DINO ViT-S/16", vit.dino_vit_config())):
        m = vit.VisionTransformer(cfg)
        with torch.no_grad():
            for n, p in m.named_parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.02 + (1.0 if "norm" in n and n.endswith("weight") else 0.0))
        models[name] = m.to(dev).eval()
    print(f"# {B} uint8 images {SIDE} x {SIDE}; us per call, median of {ROUNDS} rounds [min max], the two forms interleaved; HBM roof {HBM_PEAK / 1e12:.1f} TB/s (spec)")
    print(f"# {'af_vit_patch_rows':<16} {'MB moved':>9} | {'HIP kernel us':>14} {'GB/s':>7} {'of roof':>8} {'[min max]':>16} | {'torch ops us':>13} {'[min max]':>18} | max diff")
    for name, m in models.items():
        c = m.config
        nbytes = img.numel() + B * m.num_patches * m.patch_kcols() * 2
        diff = (m.patch_rows(img).float() - torch_rows(img, c, m.patch_kcols()).float()).abs().max().item()
        th, tr = compare(lambda: m.patch_rows(img), lambda: torch_rows(img, c, m.patch_kcols()), 20)
        mh, mr = th[ROUNDS // 2], tr[ROUNDS // 2]
        print(f"  {name:<16} {nbytes / 1e6:9.1f} | {mh:14.1f} {nbytes / mh * 1e-3:7.0f} {nbytes / (mh * 1e-6) / HBM_PEAK:8.1%} {f'[{th[0]:.1f} {th[-1]:.1f}]':>16} | {mr:13.1f} "
              f"{f'[{tr[0]:.1f} {tr[-1]:.1f}]':>18} | {diff:.2e}", flush=True)
    print(f"# {'whole encoder':<16} | {'HIP path img/s':>14} {'ms':>8} {'[min max] ms':>18} | {'torch fp16 img/s':>16} {'ms':>8} {'[min max] ms':>18} | feature rel-L2")
    with torch.no_grad():
        for name, m in models.items():
            a, b = m.forward_u8(img).float(), torch_encoder(m, img).float()
            rel = float((a - b).norm() / b.norm())
            th, tr = compare(lambda: m.forward_u8(img), lambda: torch_encoder(m, img), 5)
            mh, mr = th[ROUNDS // 2], tr[ROUNDS // 2]
            print(f"  {name:<16} | {B / mh * 1e6:14.0f} {mh / 1e3:8.2f} {f'[{th[0] / 1e3:.2f} {th[-1] / 1e3:.2f}]':>18} | {B / mr * 1e6:16.0f} {mr / 1e3:8.2f} "
                  f"{f'[{tr[0] / 1e3:.2f} {tr[-1] / 1e3:.2f}]':>18} | {rel:.2e}", flush=True)


if __name__ == "__main__":
    main()
