"""SD-1.5 U-Net LoRA loading and fusing (e.g. LCM-LoRA, ``latent-consistency/lcm-lora-sdv1-5``).

``unet_name_map(unet_config)`` maps every diffusers U-Net module that carries a weight (282 on the SD-1.5 topology) to its path in this
package's LDM module tree, by the rules of diffusers' LDM <-> diffusers checkpoint conversion.  ``read_unet_lora`` turns a LoRA file
or state dict in any of three layouts into ``{ldm_path: (down, up, alpha | None)}``:

* kohya:            ``lora_unet_<diffusers path, "." -> "_">.lora_down.weight`` / ``.lora_up.weight`` / ``.alpha``
* diffusers legacy: ``unet.<diffusers path>.lora.down.weight`` / ``.lora.up.weight``
* peft:             ``unet.<diffusers path>.lora_A.weight`` / ``.lora_B.weight``

A kohya path is decoded through a table built from the name map (an underscore cannot be split on).  Keys that map to nothing
(text-encoder LoRA, unknown layers), down / up shapes that do not fit the layer and half pairs are refused with ``ValueError``.

``fuse_unet_lora`` computes W' = W + scale * (alpha / r, or 1 without alpha) * up @ down in fp32 through
``autograd_ops.low_rank_product`` (the package's GEMM on the device) and writes it with an in-place ``copy_``, as
``lora.merge_unet_loras`` does: every packed fp16 cache keyed on the parameter's version (the concatenated q|k|v and k|v, the one
[sum Cout, 1280] emb_layers matrix, the interleaved GEGLU rows) is rebuilt on the next call.  ``unfuse_unet_lora`` restores the saved
originals bit-exactly.  A graph captured before a fuse still replays the old packs: do not replay it afterwards."""
import os

import torch

from .lora import _get

RESNET_LEAVES = {"conv1": "in_layers.2", "conv2": "out_layers.3", "time_emb_proj": "emb_layers.1", "conv_shortcut": "skip_connection"}
TRANSFORMER_LEAVES = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v",
                      "attn2.to_out.0", "ff.net.0.proj", "ff.net.2")
NON_LORA_TARGETS = ("conv_in", "conv_out", "time_embedding.linear_1", "time_embedding.linear_2")


def unet_name_map(unet_config):
    """{diffusers module path: LDM module path} of every Conv2d / Linear of UNetModel(**unet_config) (spatial-transformer topology)."""
    nrb = unet_config["num_res_blocks"]
    mult = list(unet_config["channel_mult"])
    depth = unet_config.get("transformer_depth", 1)
    levels = len(mult)
    attn = [2 ** i in unet_config["attention_resolutions"] for i in range(levels)]
    m = {"conv_in": "input_blocks.0.0", "conv_out": "out.2", "time_embedding.linear_1": "time_embed.0",
         "time_embedding.linear_2": "time_embed.2"}

    def resnet(d, l, shortcut):
        for dl, ll in RESNET_LEAVES.items():
            if dl != "conv_shortcut" or shortcut:
                m[f"{d}.{dl}"] = f"{l}.{ll}"

    def transformer(d, l):
        m[f"{d}.proj_in"], m[f"{d}.proj_out"] = f"{l}.proj_in", f"{l}.proj_out"
        for k in range(depth):
            for leaf in TRANSFORMER_LEAVES:
                m[f"{d}.transformer_blocks.{k}.{leaf}"] = f"{l}.transformer_blocks.{k}.{leaf}"

    prev = 1
    for i in range(levels):
        for j in range(nrb):
            blk = (nrb + 1) * i + j + 1
            resnet(f"down_blocks.{i}.resnets.{j}", f"input_blocks.{blk}.0", j == 0 and mult[i] != prev)
            if attn[i]:
                transformer(f"down_blocks.{i}.attentions.{j}", f"input_blocks.{blk}.1")
        if i < levels - 1:
            m[f"down_blocks.{i}.downsamplers.0.conv"] = f"input_blocks.{(nrb + 1) * i + nrb + 1}.0.op"
        prev = mult[i]
    resnet("mid_block.resnets.0", "middle_block.0", False)
    transformer("mid_block.attentions.0", "middle_block.1")
    resnet("mid_block.resnets.1", "middle_block.2", False)
    for i in range(levels):
        level = levels - 1 - i
        for j in range(nrb + 1):
            blk = (nrb + 1) * i + j
            resnet(f"up_blocks.{i}.resnets.{j}", f"output_blocks.{blk}.0", True)       # the skip concatenation widens every input
            if attn[level]:
                transformer(f"up_blocks.{i}.attentions.{j}", f"output_blocks.{blk}.1")
        if i < levels - 1:
            m[f"up_blocks.{i}.upsamplers.0.conv"] = f"output_blocks.{(nrb + 1) * i + nrb}.{2 if attn[level] else 1}.conv"
    return m


def lora_target_map(unet_config):
    """The name map without conv_in, conv_out and the time embedding: the layers an SD-1.5 U-Net LoRA such as LCM-LoRA targets
    (278 on the SD-1.5 topology)."""
    return {d: l for d, l in unet_name_map(unet_config).items() if d not in NON_LORA_TARGETS}


def kohya_table(name_map):
    """{kohya module name ``lora_unet_<path with . -> _>``: diffusers path}; raises if two paths collide."""
    t = {}
    for d in name_map:
        k = "lora_unet_" + d.replace(".", "_")
        if k in t:
            raise ValueError(f"kohya names of {t[k]!r} and {d!r} collide")
        t[k] = d
    return t


def load_lora_file(path):
    """A LoRA state dict from ``.safetensors`` or a torch file (``.bin`` / ``.pt``, loaded with weights_only=True)."""
    if os.path.splitext(path)[1] == ".safetensors":
        from safetensors.torch import load_file
        return load_file(path)
    return torch.load(path, map_location="cpu", weights_only=True)


_SUFFIXES = (  # (layout, key prefix, key suffix, slot)
    ("kohya", "lora_unet_", ".lora_down.weight", "down"), ("kohya", "lora_unet_", ".lora_up.weight", "up"),
    ("kohya", "lora_unet_", ".alpha", "alpha"),
    ("legacy", "unet.", ".lora.down.weight", "down"), ("legacy", "unet.", ".lora.up.weight", "up"),
    ("peft", "unet.", ".lora_A.weight", "down"), ("peft", "unet.", ".lora_B.weight", "up"),
)


def unet_config_of(unet):
    """The topology entries of the config a UNetModel was built from (what unet_name_map reads)."""
    st = next((m for m in unet.modules() if hasattr(m, "transformer_blocks")), None)
    return dict(num_res_blocks=unet.num_res_blocks, channel_mult=list(unet.channel_mult),
                attention_resolutions=list(unet.attention_resolutions), transformer_depth=len(st.transformer_blocks) if st else 1)


def read_unet_lora(path_or_state_dict, model):
    """{ldm_path: (down [r, Cin(, kh, kw)], up [Cout, r(, 1, 1)], alpha float | None)} of a LoRA file or state dict in the kohya,
    diffusers-legacy or peft layout, checked against the layers of ``model`` (a UNetWrapper, or the UNetModel itself)."""
    unet = getattr(model, "diffusion_model", model)
    sd = load_lora_file(path_or_state_dict) if isinstance(path_or_state_dict, (str, os.PathLike)) else path_or_state_dict
    name_map = lora_target_map(unet_config_of(unet))
    kohya = kohya_table(name_map)
    parts, unknown = {}, []
    for key, val in sd.items():
        for layout, prefix, suffix, slot in _SUFFIXES:
            if key.startswith(prefix) and key.endswith(suffix):
                mod = key[:-len(suffix)]
                d = kohya.get(mod) if layout == "kohya" else mod[len(prefix):]
                if d in name_map:
                    parts.setdefault(name_map[d], {}).setdefault(slot, []).append((key, val))
                    break
        else:
            unknown.append(key)
    if unknown:
        raise ValueError(f"{len(unknown)} LoRA keys map to no U-Net layer of this model (only U-Net LoRA in the kohya, diffusers or "
                         f"peft layout is read; text-encoder LoRA is not), e.g. {unknown[:5]}")
    out = {}
    for lpath, p in parts.items():
        keys = [k for v in p.values() for k, _ in v]
        if any(len(v) > 1 for v in p.values()):
            raise ValueError(f"layer {lpath} appears more than once in the LoRA state dict: {keys}")
        if "down" not in p or "up" not in p:
            raise ValueError(f"incomplete LoRA pair for layer {lpath}: only {keys}")
        down, up = p["down"][0][1], p["up"][0][1]
        w = _get(unet, lpath).weight
        r = down.shape[0] if down.dim() >= 1 else 0
        if r < 1 or tuple(down.shape) != (r,) + tuple(w.shape[1:]) or tuple(up.shape) != (w.shape[0], r) + (1,) * (w.dim() - 2):
            raise ValueError(f"LoRA shapes down {tuple(down.shape)} / up {tuple(up.shape)} do not fit layer {lpath} with weight "
                             f"{tuple(w.shape)} (want down [r, {', '.join(map(str, w.shape[1:]))}], up [{w.shape[0]}, r"
                             f"{', 1, 1' if w.dim() == 4 else ''}])")
        alpha = float(p["alpha"][0][1]) if "alpha" in p else None
        out[lpath] = (down, up, alpha)
    return out


def check_no_live_merge(model):
    """Fusing and unfusing refuse while an AdaFace DoRA merge is live (its saved originals would be restored over the fused weights)."""
    if getattr(model, "_merge_saved", None):
        raise RuntimeError("an AdaFace DoRA adapter merge is live on this U-Net (UNetWrapper._merge_saved): switch the adapters off "
                           "before fusing or unfusing a LoRA")


@torch.no_grad()
def fuse_unet_lora(model, lora, scale=1.0):
    """Fuse ``lora`` (read_unet_lora's dict) into ``model`` (a UNetWrapper, or the UNetModel itself) in place:
    W' = W + scale * (alpha / r or 1) * up @ down in fp32.  Returns {ldm_path: original weight} for unfuse_unet_lora."""
    from ..autograd_ops import low_rank_product
    check_no_live_merge(model)
    unet = getattr(model, "diffusion_model", model)
    saved = {}
    for lpath, (down, up, alpha) in lora.items():
        w = _get(unet, lpath).weight
        r = down.shape[0]
        a, b = down.to(w.device, torch.float32).flatten(1), up.to(w.device, torch.float32).flatten(1)
        if w.is_cuda and r % 8:                      # zero rank padding keeps the product on the package's GEMM (rank multiple of 8)
            pad = 8 - r % 8
            a, b = torch.cat([a, a.new_zeros(pad, a.shape[1])]), torch.cat([b, b.new_zeros(b.shape[0], pad)], dim=1)
        delta = low_rank_product(b, a).reshape(w.shape)
        saved[lpath] = w.detach().clone()
        w.copy_((w.float() + (scale * (alpha / r if alpha is not None else 1.0)) * delta).to(w.dtype))
    return saved


@torch.no_grad()
def unfuse_unet_lora(model, saved):
    """Restore the originals saved by fuse_unet_lora (bit-exact)."""
    check_no_live_merge(model)
    unet = getattr(model, "diffusion_model", model)
    for lpath, w in saved.items():
        _get(unet, lpath).weight.copy_(w)
