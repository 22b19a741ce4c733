"""Shared by the ControlNet tests: a synthetic cldm-layout state dict for a U-Net config, an fp64 hint encoder and a plain-torch CPU walk of
U-Net + ControlNet (composed from oracle.unet_oracle's layer functions, as motion_util.unet_forward_video is; oracle/ itself knows nothing
of ControlNet).  The walk restates cldm's ControlNet.forward / ControlledUnetModel.forward: the hint features are added behind conv_in, every
input block's output and the middle block's go through a 1x1 "zero convolution", and the U-Net adds scale x those to its middle output
and, popping, to its skips.  With a motion state dict the U-Net runs AnimateDiff's temporal transformers and the ControlNet runs per frame.

Real zero convolutions are trained away from zero; the synthetic ones are drawn like every other weight and multiplied by ``zero_gain``,
the dial of the sensitivity conditions in test_controlnet_host.py."""
import torch
import torch.nn.functional as F

from adaface_dev_amd import rng
from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import unet_param_shapes
from motion_util import HEADS, temporal_transformer_ref
from oracle import unet_oracle as O

HINT_LAYERS = [(3, 16, 1), (16, 16, 1), (16, 32, 2), (32, 32, 1), (32, 96, 2), (96, 96, 1), (96, 256, 2)]    # input_hint_block.{0,..,12}
# Gains of the three kinds of convolution cldm initialises to zero, all asserted sufficient in test_controlnet_host.py::test_reference_teeth:
# the twelve zero_convs, middle_block_out, and the hint encoder's last convolution (behind seven unit-gain SiLU layers on an image in [0, 1]
# the hint would otherwise be ~2 % of conv_in's output and a wrong hint invisible).
ZERO_GAIN, MID_GAIN, HINT_GAIN = 1.0, 2.0, 16.0
FAULTS = ("no_hint", "no_mid", "drop_zero", "swap_skips", "no_silu")


def block_channels(cfg):
    """Output channels of the twelve (3 n_levels) input blocks."""
    mc, out = cfg["model_channels"], [cfg["model_channels"]]
    for level, mult in enumerate(cfg["channel_mult"]):
        out += [mc * mult] * cfg["num_res_blocks"]
        if level != len(cfg["channel_mult"]) - 1:
            out.append(mc * mult)
    return out


def controlnet_shapes(cfg):
    """{key: shape} of cldm.ControlNet for the U-Net of cfg: the U-Net's own encoder keys plus the hint block and the zero convolutions."""
    s = {n: shape for n, shape in unet_param_shapes(cfg) if n.startswith(("time_embed.", "input_blocks.", "middle_block."))}
    for k, (cin, cout, _) in enumerate(HINT_LAYERS):
        s[f"input_hint_block.{2 * k}.weight"], s[f"input_hint_block.{2 * k}.bias"] = (cout, cin, 3, 3), (cout,)
    s["input_hint_block.14.weight"], s["input_hint_block.14.bias"] = (cfg["model_channels"], 256, 3, 3), (cfg["model_channels"],)
    chans = block_channels(cfg)
    for i, c in enumerate(chans):
        s[f"zero_convs.{i}.0.weight"], s[f"zero_convs.{i}.0.bias"] = (c, c, 1, 1), (c,)
    s["middle_block_out.0.weight"], s["middle_block_out.0.bias"] = (chans[-1], chans[-1], 1, 1), (chans[-1],)
    return s


def synth_controlnet_sd(cfg, seed=17, zero_gain=ZERO_GAIN, mid_gain=MID_GAIN, hint_gain=HINT_GAIN, prefix=""):
    sd = {}
    for k, shape in controlnet_shapes(cfg).items():
        t = rng.synth_tensor("controlnet." + k, shape, seed).clone()
        gain = zero_gain if k.startswith("zero_convs.") else mid_gain if k.startswith("middle_block_out.") else \
            hint_gain if k == "input_hint_block.14.weight" else 1.0
        sd[prefix + k] = t * gain
    return sd


def synth_control_images(B0, H, W, seed=3):
    """uint8 [B0, H, W, 3]: per image its own stripes (direction, period, colour) on its own brightness, plus noise; the byte range is used
    in full, and the images differ enough that a hint given to the wrong row shows."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    imgs = []
    for b in range(B0):
        wave = torch.sin((xx if b % 2 else yy) * (0.35 + 0.25 * b) + b)
        colour = torch.tensor([[1.0, 0.2, 0.6], [0.1, 1.0, 0.4], [0.5, 0.3, 1.0]][b % 3])
        level = 0.25 + 0.5 * (b % 2)
        imgs.append((level + 0.45 * wave[..., None] * colour) * 255)
    img = torch.stack(imgs) + 30 * torch.randn(B0, H, W, 3, generator=g)
    return img.clamp(0, 255).round().to(torch.uint8)


def hint_encoder_ref(csd, images_u8, dt=torch.float64, silu=True, round_f16=False):
    """input_hint_block on images / 255 in dtype dt -> [B0, model_channels, h, w].  round_f16: every tensor the device stores (the seven
    activations and the output; weights as they are packed) rounded to fp16."""
    r = (lambda t: t.half().to(dt)) if round_f16 else (lambda t: t)
    x = (images_u8.to(dt) / torch.tensor(255.0, dtype=dt)).permute(0, 3, 1, 2)
    for k, (_, _, stride) in enumerate(HINT_LAYERS):
        x = F.conv2d(x, r(csd[f"input_hint_block.{2 * k}.weight"].to(dt)), csd[f"input_hint_block.{2 * k}.bias"].to(dt), stride=stride, padding=1)
        x = r(F.silu(x) if silu else x)
    return r(F.conv2d(x, r(csd["input_hint_block.14.weight"].to(dt)), csd["input_hint_block.14.bias"].to(dt), padding=1))


def _emb(sd, cfg, timesteps):
    t_emb = O.timestep_embedding(timesteps, cfg["model_channels"])
    emb = F.linear(t_emb, sd["time_embed.0.weight"], sd["time_embed.0.bias"])
    return F.linear(F.silu(emb), sd["time_embed.2.weight"], sd["time_embed.2.bias"])


def _layer(sd, cfg, emb, context, kind, p, h):
    if kind == "conv_in":
        return O.conv2d(h, sd[p + "weight"], sd[p + "bias"])
    if kind == "res":
        return O.res_block(sd, p, h, emb)
    if kind == "attn":
        return O.spatial_transformer(sd, p, h, context, None, cfg["num_heads"])
    if kind == "down":
        return O.conv2d(h, sd[p + "op.weight"], sd[p + "op.bias"], stride=2)
    h = F.interpolate(h, scale_factor=2, mode="nearest")
    return O.conv2d(h, sd[p + "conv.weight"], sd[p + "conv.bias"])


def controlnet_residuals(csd, cfg, x, timesteps, context, hint):
    """cldm ControlNet.forward: -> the thirteen zero-convolution outputs (twelve input blocks, then the middle block), unscaled.
    hint [B, model_channels, h, w] or None (a dropped hint)."""
    inputs, middle, _ = O.unet_topology(cfg)
    emb = _emb(csd, cfg, timesteps)
    h, outs = x.float(), []
    for n, layers in enumerate(inputs):
        for kind, p in layers:
            h = _layer(csd, cfg, emb, context, kind, p, h)
        if n == 0 and hint is not None:
            h = h + hint
        outs.append(F.conv2d(h, csd[f"zero_convs.{n}.0.weight"], csd[f"zero_convs.{n}.0.bias"]))
    for kind, p in middle:
        h = _layer(csd, cfg, emb, context, kind, p, h)
    outs.append(F.conv2d(h, csd["middle_block_out.0.weight"], csd["middle_block_out.0.bias"]))
    return outs


def unet_forward_control(sd, csd, cfg, x, timesteps, context, images_u8=None, scale=1.0, msd=None, nf=1, fault=None, hint=None):
    """eps of the U-Net of ``sd`` under the ControlNet of ``csd`` (None: the plain walk) on control images uint8 [B0, 8h, 8w, 3]; row b takes
    image b % B0.  ``hint``: precomputed hint_encoder_ref(...).float() instead of the images.  ``msd``: a motion-module state dict for
    videos of ``nf`` frames.  ``fault``: one of FAULTS, a deliberately wrong walk for the sensitivity tests."""
    assert fault is None or fault in FAULTS
    inputs, middle, outputs = O.unet_topology(cfg)
    emb = _emb(sd, cfg, timesteps)

    def motion(prefix, h):
        p = prefix + ".temporal_transformer."
        return temporal_transformer_ref(msd, p, h, nf, heads=HEADS) if msd is not None and (p + "norm.weight") in msd else h

    h, hs = x.float(), []
    for n, layers in enumerate(inputs):
        for kind, p in layers:
            h = _layer(sd, cfg, emb, context, kind, p, h)
        if n % 3 and n <= 11:
            h = motion(f"down_blocks.{(n - 1) // 3}.motion_modules.{(n - 1) % 3}", h)
        hs.append(h)
    res = None
    if csd is not None:
        if hint is None:
            hint = hint_encoder_ref(csd, images_u8, torch.float64, silu=fault != "no_silu").float()
        B = x.shape[0]
        assert B % hint.shape[0] == 0
        hint_b = None if fault == "no_hint" else hint.repeat(B // hint.shape[0], 1, 1, 1)
        res = controlnet_residuals(csd, cfg, x, timesteps, context, hint_b)
        if fault == "drop_zero":
            res[4] = torch.zeros_like(res[4])
        if fault == "swap_skips":
            assert res[4].shape == res[5].shape
            res[4], res[5] = res[5], res[4]
        if fault == "no_mid":
            res[12] = torch.zeros_like(res[12])
        hs = [s + scale * r for s, r in zip(hs, res[:12])]
    for k, (kind, p) in enumerate(middle):
        if k == 2:
            h = motion("mid_block.motion_modules.0", h)
        h = _layer(sd, cfg, emb, context, kind, p, h)
    if res is not None:
        h = h + scale * res[12]
    for n, layers in enumerate(outputs):
        h = torch.cat([h, hs.pop()], dim=1)
        done = False
        for kind, p in layers:
            if kind == "up":
                h, done = motion(f"up_blocks.{n // 3}.motion_modules.{n % 3}", h), True
            h = _layer(sd, cfg, emb, context, kind, p, h)
        if not done:
            h = motion(f"up_blocks.{n // 3}.motion_modules.{n % 3}", h)
    h = O.group_norm(h, sd["out.0.weight"], sd["out.0.bias"], 1e-5, silu=True)
    return O.conv2d(h, sd["out.2.weight"], sd["out.2.bias"])
