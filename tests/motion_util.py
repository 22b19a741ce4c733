"""Shared by the motion-module tests: synthetic AnimateDiff state dicts and a plain-torch fp32 CPU restatement of the temporal transformer
and of the U-Net walk with motion modules (composed from oracle.unet_oracle's layer functions; oracle/ itself knows nothing of video)."""
import math

import torch
import torch.nn.functional as F

from adaface_dev_amd import TINY_UNET_CONFIG, rng
from oracle import unet_oracle as O

HEADS = 8


def motion_unet_cfg():
    """The reduced-width U-Net of the wrapper tests: head dims 8 / 16 / 32 / 32."""
    return dict(TINY_UNET_CONFIG, model_channels=64, context_dim=128)


def direct_pe(max_len, C):
    """The position table evaluated entry by entry in fp64: pe[pos, 2i] = sin(pos e^(-2i ln 10000 / C)), pe[pos, 2i+1] = cos(same)."""
    pe = torch.zeros(1, max_len, C, dtype=torch.float64)
    for pos in range(max_len):
        for i in range(0, C, 2):
            a = pos * math.exp(-i * math.log(10000.0) / C)
            pe[0, pos, i] = math.sin(a)
            if i + 1 < C:
                pe[0, pos, i + 1] = math.cos(a)
    return pe


def prefix_channels(cfg):
    """{key prefix: channels} of the 21 placements on a 4-level, 2-ResBlock U-Net."""
    mc, mult = cfg["model_channels"], cfg["channel_mult"]
    out = {}
    for i in range(4):
        for j in range(2):
            out[f"down_blocks.{i}.motion_modules.{j}"] = mc * mult[i]
    out["mid_block.motion_modules.0"] = mc * mult[3]
    for i in range(4):
        for j in range(3):
            out[f"up_blocks.{i}.motion_modules.{j}"] = mc * mult[3 - i]
    return out


def transformer_shapes(C, max_len):
    s = {"norm.weight": (C,), "norm.bias": (C,), "proj_in.weight": (C, C), "proj_in.bias": (C,), "proj_out.weight": (C, C), "proj_out.bias": (C,)}
    b = "transformer_blocks.0."
    for k in range(2):
        a = f"{b}attention_blocks.{k}."
        s.update({a + "to_q.weight": (C, C), a + "to_k.weight": (C, C), a + "to_v.weight": (C, C), a + "to_out.0.weight": (C, C),
                  a + "to_out.0.bias": (C,), a + "pos_encoder.pe": (1, max_len, C)})
        s.update({f"{b}norms.{k}.weight": (C,), f"{b}norms.{k}.bias": (C,)})
    s.update({b + "ff.net.0.proj.weight": (8 * C, C), b + "ff.net.0.proj.bias": (8 * C,), b + "ff.net.2.weight": (C, 4 * C),
              b + "ff.net.2.bias": (C,), b + "ff_norm.weight": (C,), b + "ff_norm.bias": (C,)})
    return s


def synth_motion_sd(cfg, with_mid=True, max_len=32, seed=5):
    """A synthetic motion-module state dict in AnimateDiff's key layout: weights from rng.synth_tensor, pe the sinusoidal table."""
    sd = {}
    for prefix, C in prefix_channels(cfg).items():
        if prefix.startswith("mid_block") and not with_mid:
            continue
        for name, shape in transformer_shapes(C, max_len).items():
            key = f"{prefix}.temporal_transformer.{name}"
            sd[key] = direct_pe(max_len, C).float() if name.endswith("pos_encoder.pe") else rng.synth_tensor(key, shape, seed).clone()
    return sd


def temporal_transformer_ref(msd, p, x, nf, heads=HEADS):
    """x [B*F, C, H, W] fp32 (video-major) -> same shape.  p: key prefix up to and including 'temporal_transformer.'."""
    BF, C, H, W = x.shape
    B = BF // nf
    y = O.group_norm(x, msd[p + "norm.weight"], msd[p + "norm.bias"], 1e-6)
    y = y.reshape(B, nf, C, H * W).permute(0, 3, 1, 2).reshape(B * H * W, nf, C)               # one sequence per pixel
    h = F.linear(y, msd[p + "proj_in.weight"], msd[p + "proj_in.bias"])
    b = p + "transformer_blocks.0."
    for k in range(2):
        a = f"{b}attention_blocks.{k}."
        n = F.layer_norm(h, (C,), msd[f"{b}norms.{k}.weight"], msd[f"{b}norms.{k}.bias"], 1e-5) + msd[a + "pos_encoder.pe"][:, :nf]
        q, kk, v = (F.linear(n, msd[a + f"to_{t}.weight"]) for t in "qkv")
        h = h + F.linear(O.attention_core(q, kk, v, heads), msd[a + "to_out.0.weight"], msd[a + "to_out.0.bias"])
    h = h + O.geglu_ff(msd, b + "ff.", F.layer_norm(h, (C,), msd[b + "ff_norm.weight"], msd[b + "ff_norm.bias"], 1e-5))
    h = F.linear(h, msd[p + "proj_out.weight"], msd[p + "proj_out.bias"])
    return x + h.reshape(B, H * W, nf, C).permute(0, 2, 3, 1).reshape(BF, C, H, W)


def unet_forward_video(sd, msd, cfg, x, timesteps, context, nf):
    """The U-Net walk of oracle.unet_oracle.unet_forward with the temporal transformers of ``msd`` at AnimateDiff's places (``msd`` None: the
    image walk).  The skip pushed for an input block is the tensor behind its motion module."""
    heads = cfg["num_heads"]
    inputs, middle, outputs = O.unet_topology(cfg)
    t_emb = O.timestep_embedding(timesteps, cfg["model_channels"])
    emb = F.linear(t_emb, sd["time_embed.0.weight"], sd["time_embed.0.bias"])
    emb = F.linear(F.silu(emb), sd["time_embed.2.weight"], sd["time_embed.2.bias"])

    def motion(prefix, h):
        p = prefix + ".temporal_transformer."
        return temporal_transformer_ref(msd, p, h, nf, heads=HEADS) if msd is not None and (p + "norm.weight") in msd else h

    def layer(kind, p, h):
        if kind == "conv_in":
            return O.conv2d(h, sd[p + "weight"], sd[p + "bias"])
        if kind == "res":
            return O.res_block(sd, p, h, emb)
        if kind == "attn":
            return O.spatial_transformer(sd, p, h, context, None, heads)
        if kind == "down":
            return O.conv2d(h, sd[p + "op.weight"], sd[p + "op.bias"], stride=2)
        h = F.interpolate(h, scale_factor=2, mode="nearest")
        return O.conv2d(h, sd[p + "conv.weight"], sd[p + "conv.bias"])

    h, hs = x.float(), []
    for n, layers in enumerate(inputs):
        for kind, p in layers:
            h = layer(kind, p, h)
        if n % 3 and n <= 11:                                    # input_blocks[3i + 1 + j]
            h = motion(f"down_blocks.{(n - 1) // 3}.motion_modules.{(n - 1) % 3}", h)
        hs.append(h)
    for k, (kind, p) in enumerate(middle):
        if k == 2:
            h = motion("mid_block.motion_modules.0", h)
        h = layer(kind, p, h)
    for n, layers in enumerate(outputs):
        h = torch.cat([h, hs.pop()], dim=1)
        done = False
        for kind, p in layers:
            if kind == "up":
                h, done = motion(f"up_blocks.{n // 3}.motion_modules.{n % 3}", h), True
            h = layer(kind, p, h)
        if not done:
            h = motion(f"up_blocks.{n // 3}.motion_modules.{n % 3}", h)
    h = O.group_norm(h, sd["out.0.weight"], sd["out.0.bias"], 1e-5, silu=True)
    return O.conv2d(h, sd["out.2.weight"], sd["out.2.bias"])
