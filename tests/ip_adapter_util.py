"""Shared by the IP-Adapter tests: a synthetic published-layout state dict for a U-Net config and a plain-torch CPU restatement of the adapter
(image projection, decoupled cross-attention) inside the U-Net walk of controlnet_util (itself composed from oracle.unet_oracle's layer
functions; oracle/ knows nothing of IP-Adapter).  The walk restates tencent-ailab/IP-Adapter's IPAttnProcessor: in every cross-attention
layer ``o = attn(q, k_text, v_text) + scale * attn(q, to_k_ip(tokens), to_v_ip(tokens))`` in front of to_out, the file's ``{i}`` keys read
in diffusers' attn_processors order (down blocks, up blocks, mid).

The published to_v_ip are trained; the synthetic ones are drawn like every other weight and multiplied by ``V_GAIN`` (``MID_GAIN`` more for
two of them), the dials of the sensitivity conditions in test_ip_adapter_host.py."""
import contextlib

import torch
import torch.nn.functional as F

import controlnet_util as CU
from adaface_dev_amd import rng
from adaface_dev_amd.adaface import ip_adapter as IP
from oracle import unet_oracle as O

V_GAIN = 4.0
MID_GAIN = 4.0                   # on top of V_GAIN for keys 13 and 31 (the first up layer and the middle block): the middle block is one layer of 16 on
                                 # the smallest map, and a table that confuses the two must still move eps by ten times the GPU tolerance
LORA_RANK = 8                    # the synthetic FaceID LoRA pairs (the published ones have rank 128; the loader reads the rank from the file)
LORA_GAIN = 0.5
FAULTS = ("no_ip", "shared_softmax", "swap_cond_uncond", "mid_last_wrong", "no_norm")
# the wrong table of fault "mid_last_wrong": the middle block reads i = 13 (where a down, mid, up enumeration would put it; the first up layer has
# the middle block's width) instead of 31, the last
SEQUENTIAL_INDEX = tuple(13 if i == 31 else i for i in IP.KEY_INDEX)


def synth_ip_sd(cfg, kind, num_tokens=4, seed=23, v_gain=V_GAIN, nested=True, mid_gain=MID_GAIN):
    """A synthetic file of ``kind`` for the U-Net of cfg: {"image_proj": {...}, "ip_adapter": {...}} (nested) or the prefixed flat spelling."""
    flat = {}
    for k, shape in IP.expected_shapes(cfg, kind, num_tokens, LORA_RANK).items():
        t = rng.synth_tensor(f"ip.{kind}." + k, shape, seed).clone()
        if k.endswith(".to_v_ip.weight"):
            t = t * v_gain * (mid_gain if k.split(".")[1] in ("13", "31") else 1.0)
        if "_lora." in k:
            t = t * LORA_GAIN
        flat[k] = t
    if not nested:
        return flat
    return {part: {k[len(part) + 1:]: v for k, v in flat.items() if k.startswith(part + ".")} for part in ("image_proj", "ip_adapter")}


def flat_sd(sd):
    return IP._flatten(sd)


def image_proj_ref(sd, kind, embeds, num_tokens=4, dt=torch.float64, norm=True):
    """image_proj of a file's state dict on embeds [B, 1024 | 512] in dtype dt -> [B, T, ctx]."""
    f = {k[len("image_proj."):]: v.to(dt) for k, v in flat_sd(sd).items() if k.startswith("image_proj.")}
    e = embeds.to(dt)
    if kind == "clip":
        y = F.linear(e, f["proj.weight"], f["proj.bias"])
    else:
        y = F.linear(F.gelu(F.linear(e, f["proj.0.weight"], f["proj.0.bias"])), f["proj.2.weight"], f["proj.2.bias"])
    ctx = f["norm.weight"].shape[0]
    y = y.reshape(e.shape[0], num_tokens, ctx)
    return F.layer_norm(y, (ctx,), f["norm.weight"], f["norm.bias"], 1e-5) if norm else y


def fused_unet_sd(sd, ipsd, cfg, lora_scale=1.0):
    """The U-Net state dict with a FaceID file's LoRA fused: W += lora_scale * up @ down (no alpha), in the weights' dtype."""
    f = flat_sd(ipsd)
    out = dict(sd)
    for key, path in IP._lora_paths(IP.cross_attn_layout(cfg)).items():
        w = sd[path + ".weight"]
        delta = f[f"ip_adapter.{key}.up.weight"].to(torch.float64) @ f[f"ip_adapter.{key}.down.weight"].to(torch.float64)
        out[path + ".weight"] = (w.to(torch.float64) + lora_scale * delta).to(w.dtype)
    return out


def ip_block(sd, p, x, context, heads, wk, wv, tokens, scale, shared_softmax=False):
    """BasicTransformerBlock._forward (O.basic_transformer_block) with the image tokens' attention added to attn2's core."""
    C = x.shape[-1]
    ln = lambda t, n: F.layer_norm(t, (C,), sd[p + n + ".weight"], sd[p + n + ".bias"], 1e-5)
    x1 = O.cross_attention(sd, p + "attn1.", ln(x, "norm1"), None, None, heads) + x
    xn = ln(x1, "norm2")
    q = F.linear(xn, sd[p + "attn2.to_q.weight"])
    k, v = F.linear(context, sd[p + "attn2.to_k.weight"]), F.linear(context, sd[p + "attn2.to_v.weight"])
    kip, vip = F.linear(tokens, wk.to(x.dtype)), F.linear(tokens, wv.to(x.dtype))
    if shared_softmax:
        core = O.attention_core(q, torch.cat([k, kip], 1), torch.cat([v, scale * vip], 1), heads)
    else:
        core = O.attention_core(q, k, v, heads) + scale * O.attention_core(q, kip, vip, heads)
    x2 = x1 + F.linear(core, sd[p + "attn2.to_out.0.weight"], sd[p + "attn2.to_out.0.bias"])
    return O.geglu_ff(sd, p + "ff.", ln(x2, "norm3")) + x2


def ip_spatial_transformer(sd, p, x, context, heads, wk, wv, tokens, scale, shared_softmax=False):
    """O.spatial_transformer with ip_block in place of the plain block, in x's dtype (O.group_norm computes in fp32; for fp32 x this is it)."""
    b, c, h, w = x.shape
    y = F.group_norm(x, 32, sd[p + "norm.weight"], sd[p + "norm.bias"], 1e-6)
    y = O.conv2d(y, sd[p + "proj_in.weight"], sd[p + "proj_in.bias"], padding=0)
    y = y.permute(0, 2, 3, 1).reshape(b, h * w, c)
    y = ip_block(sd, p + "transformer_blocks.0.", y, context, heads, wk, wv, tokens, scale, shared_softmax)
    y = y.reshape(b, h, w, c).permute(0, 3, 1, 2)
    return O.conv2d(y, sd[p + "proj_out.weight"], sd[p + "proj_out.bias"], padding=0) + x


@contextlib.contextmanager
def _ip_layers(sd, ipsd, cfg, tokens, scale, fault):
    """While active, controlnet_util's walk runs the U-Net ``sd``'s (and only its: a ControlNet passes its own state dict) attention layers
    with the image tokens."""
    f = flat_sd(ipsd)
    table = SEQUENTIAL_INDEX if fault == "mid_last_wrong" else IP.KEY_INDEX
    index = {prefix + ".": i for (prefix, _), i in zip(IP.cross_attn_layout(cfg), table)}
    plain = CU._layer

    def layer(lsd, lcfg, emb, context, kind, p, h):
        if kind != "attn" or lsd is not sd:
            return plain(lsd, lcfg, emb, context, kind, p, h)
        i = index[p]
        return ip_spatial_transformer(sd, p, h, context, cfg["num_heads"], f[f"ip_adapter.{i}.to_k_ip.weight"], f[f"ip_adapter.{i}.to_v_ip.weight"],
                                      tokens.to(h.dtype), scale, fault == "shared_softmax")
    CU._layer = layer
    try:
        yield
    finally:
        CU._layer = plain


def unet_forward_ip(sd, ipsd, cfg, x, timesteps, context, cond_tokens, uncond_tokens, scale=1.0, fault=None, csd=None, images_u8=None,
                    control_scale=1.0, msd=None, nf=1):
    """eps of the U-Net of ``sd`` with the adapter of ``ipsd`` on image tokens [rows, T, ctx]: a batch of rows runs the cond tokens, a batch of
    2 rows cond then uncond.  ``csd`` / ``images_u8`` / ``msd`` / ``nf``: a ControlNet and a motion module beside it (controlnet_util).
    ``fault``: one of FAULTS (``no_norm`` is a fault of the token path: see image_proj_ref)."""
    assert fault is None or fault in FAULTS
    rows, B = cond_tokens.shape[0], x.shape[0]
    assert B in (rows, 2 * rows)
    pair = (uncond_tokens, cond_tokens) if fault == "swap_cond_uncond" else (cond_tokens, uncond_tokens)
    tokens = pair[0] if B == rows else torch.cat(pair, 0)
    if fault == "no_ip":
        return CU.unet_forward_control(sd, csd, cfg, x, timesteps, context, images_u8, control_scale, msd, nf)
    with _ip_layers(sd, ipsd, cfg, tokens, scale, fault):
        return CU.unet_forward_control(sd, csd, cfg, x, timesteps, context, images_u8, control_scale, msd, nf)


def diffusers_cross_attn_order(cfg):
    """An independent enumeration of diffusers' ``unet.attn_processors`` for the SD-1.5 topology, written out: the module tree is walked in
    registration order -- down_blocks, up_blocks, mid_block -- and every transformer block contributes attn1 then attn2.  Returns the LDM
    path of the SpatialTransformer that owns processor i, for odd i (attn2)."""
    nrb, mult = cfg["num_res_blocks"], cfg["channel_mult"]
    levels = len(mult)
    has_attn = [2 ** lv in cfg["attention_resolutions"] for lv in range(levels)]
    names = []
    for d in range(levels):                                   # down_blocks.d.attentions.a  <->  input_blocks.(3 d + a + 1).1
        if has_attn[d]:
            for a in range(nrb):
                names.append(f"input_blocks.{(nrb + 1) * d + a + 1}.1")
    for u in range(levels):                                   # up_blocks.u.attentions.a  <->  output_blocks.(3 u + a).1, at level (levels - 1 - u)
        if has_attn[levels - 1 - u]:
            for a in range(nrb + 1):
                names.append(f"output_blocks.{(nrb + 1) * u + a}.1")
    names.append("middle_block.1")                            # mid_block.attentions.0
    return {2 * n + 1: name for n, name in enumerate(names)}


def ip_inputs(kind, rows=1, seed=51):
    """The inputs the U-Net tests share: latents [2 rows, 4, 8, 8] (cond rows, then uncond rows), timesteps, text context [2 rows, 77, 128] and the
    image embeddings [rows, 1024] (clip) or unit-norm face ids [rows, 512]."""
    x = rng.synth_input("ip.x", (2 * rows, 4, 8, 8), seed=seed)
    ctx = rng.synth_input("ip.ctx", (2 * rows, 77, 128), seed=seed + 1)
    t = torch.tensor([700, 250] * rows)[:2 * rows]
    e = rng.synth_input(f"ip.embeds.{kind}", (rows, IP.CLIP_EMBED_DIM if kind == "clip" else IP.FACE_ID_DIM), seed=seed + 2)
    if kind == "faceid":
        e = F.normalize(e, p=2, dim=-1)
    return x, t, ctx, e
