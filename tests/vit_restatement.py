"""fp64 torch restatements for the image-scoring tests: the two vision towers (CLIP, DINO ViT) with an optional patch mask, the CLIP text
tower, and the preprocess in front of them (antialiased resize, centre crop, affine, unfold to GEMM rows).  Written from openai/CLIP,
``transformers`` and torchvision, on plain torch CPU ops: nothing here imports the package's ops, so nothing in a reference comes from a
kernel.  State dicts use ``evaluation/vit.py``'s parameter names (``VisionTransformer`` / ``CLIPTextTower``)."""
import torch
import torch.nn.functional as F

FLT_MAX = torch.finfo(torch.float32).max


# ---------------------------------------------------------------------------------------------------------------------------- preprocess
def resize_geometry(H, W, keep_aspect, S, C):
    """torchvision Resize(S) + CenterCrop(C): the shorter side becomes S, the longer int(S * long / short); crop offsets int(round(.)),
    Python's round (half to even).  keep_aspect = 0: a square resize to C, no crop."""
    if not keep_aspect:
        return C, C, 0, 0
    Hr, Wr = (S, S * W // H) if H <= W else (S * H // W, S)
    return Hr, Wr, int(round((Hr - C) / 2.0)), int(round((Wr - C) / 2.0))


def preprocess_ref(img_u8, keep_aspect, S, C, filt, scale3, shift3, dtype=torch.float64):
    """uint8 [B, H, W, 3] -> [B, 3, C, C] in `dtype`: F.interpolate(antialias=True) on the 0 .. 255 values, crop, v * scale[c] + shift[c]."""
    B, H, W, _ = img_u8.shape
    Hr, Wr, top, left = resize_geometry(H, W, keep_aspect, S, C)
    x = img_u8.permute(0, 3, 1, 2).to(dtype)
    y = F.interpolate(x, size=(Hr, Wr), mode=("bilinear", "bicubic")[filt], antialias=True, align_corners=False)
    y = y[:, :, top:top + C, left:left + C]
    sc = torch.tensor(scale3, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    sh = torch.tensor(shift3, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    return y * sc + sh, y


def rows_ref(pix, p, kpad):
    """[B, 3, C, C] -> [B * (C / p)^2, kpad]: column c p^2 + dy p + dx (the flatten order of a conv weight [E, 3, p, p]), zeros behind 3 p^2."""
    B = pix.shape[0]
    u = F.unfold(pix, kernel_size=p, stride=p).transpose(1, 2)                # [B, P, 3 p^2], patches row-major
    out = torch.zeros((B * u.shape[1], kpad), dtype=pix.dtype)
    out[:, :3 * p * p] = u.reshape(-1, 3 * p * p)
    return out


def scale_shift(mean, std):
    """The host floats a caller passes: 1 / (255 std), -mean / std, rounded to fp32 as the C ABI takes them."""
    sc = [float(torch.tensor(1.0 / (255.0 * s), dtype=torch.float32)) for s in std]
    sh = [float(torch.tensor(-m / s, dtype=torch.float32)) for m, s in zip(mean, std)]
    return sc, sh


# ---------------------------------------------------------------------------------------------------------------------------- towers
def _ln(x, sd, name, eps):
    return F.layer_norm(x, (x.shape[-1],), sd[name + ".weight"], sd[name + ".bias"], eps)


def _lin(x, sd, name):
    return F.linear(x, sd[name + ".weight"], sd.get(name + ".bias"))


def _act(x, name):
    return x * torch.sigmoid(1.702 * x) if name == "quick_gelu" else F.gelu(x)


def _layers(h, sd, prefix, n_layers, heads, eps, act, bias):
    """Pre-LN transformer blocks on h [B, T, E]; bias [B, 1, T | 1, T] is added to every score row."""
    B, T, E = h.shape
    d = E // heads
    for i in range(n_layers):
        p = f"{prefix}{i}."
        x = _ln(h, sd, p + "layer_norm1", eps)
        q, k, v = (_lin(x, sd, p + f"self_attn.{n}_proj").reshape(B, T, heads, d).transpose(1, 2) for n in "qkv")
        s = q @ k.transpose(-1, -2) * d ** -0.5
        if bias is not None:
            s = s + bias
        o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, T, E)
        h = h + _lin(o, sd, p + "self_attn.out_proj")
        x = _ln(h, sd, p + "layer_norm2", eps)
        h = h + _lin(_act(_lin(x, sd, p + "mlp.fc1"), act), sd, p + "mlp.fc2")
    return h


def to_dtype(sd, dtype=torch.float64):
    return {k: v.detach().to(dtype) for k, v in sd.items()}


def vision_forward(sd, cfg, pix, patch_mask=None):
    """pix [B, 3, C, C] (already preprocessed) -> (last_hidden_state [B, P + 1, E] as transformers defines it, features [B, D]).
    patch_mask bool [B, P]: hidden patches get a key bias of -FLT_MAX in every layer, CLS stays visible."""
    E, p = cfg.hidden_size, cfg.patch_size
    B = pix.shape[0]
    x = F.conv2d(pix, sd["patch_embedding.weight"], sd.get("patch_embedding.bias"), stride=p).flatten(2).transpose(1, 2)
    h = torch.cat([sd["class_embedding"].view(1, 1, E).expand(B, 1, E), x], dim=1) + sd["position_embedding"][None]
    if cfg.pre_layernorm:
        h = _ln(h, sd, "pre_layrnorm", cfg.layer_norm_eps)
    bias = None
    if patch_mask is not None:
        keep = torch.cat([torch.ones((B, 1), dtype=torch.bool), patch_mask], dim=1)
        bias = torch.where(keep, 0.0, -FLT_MAX).to(pix.dtype)[:, None, None, :]
    h = _layers(h, sd, "layers.", cfg.num_hidden_layers, cfg.num_attention_heads, cfg.layer_norm_eps, cfg.hidden_act, bias)
    if cfg.pool == "ln_cls":
        last = _ln(h, sd, "post_layernorm", cfg.layer_norm_eps)
        return last, last[:, 0]
    pooled = _ln(h[:, 0], sd, "post_layernorm", cfg.layer_norm_eps)
    return h, pooled @ sd["visual_projection.weight"].T


def text_forward(sd, cfg, ids):
    """ids [B, T] -> (last_hidden_state [B, T, E] after final_layer_norm, text features [B, D]): causal mask, pooled at the first EOS."""
    B, T = ids.shape
    h = sd["text_model.embeddings.token_embedding.weight"][ids] + sd["text_model.embeddings.position_embedding.weight"][:T][None]
    causal = torch.full((T, T), -FLT_MAX, dtype=h.dtype).triu(1)[None, None]
    h = _layers(h, sd, "text_model.encoder.layers.", cfg.num_hidden_layers, cfg.num_attention_heads, 1e-5, "quick_gelu", causal)
    last = _ln(h, sd, "text_model.final_layer_norm", 1e-5)
    pos = (ids == cfg.eos_token_id).int().argmax(dim=-1)
    return last, last[torch.arange(B), pos] @ sd["text_projection.weight"].T


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())
