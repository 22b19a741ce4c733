"""IP-Adapter and IP-Adapter-FaceID for the SD-1.5 U-Net: an image prompt as extra cross-attention tokens.

``IPAdapter(unet_config, kind)`` holds what the published files hold: ``image_proj`` (``kind="clip"``: ImageProjModel on the 1024-d projected
CLS of CLIP ViT-H/14; ``kind="faceid"``: MLPProjModel on the 512-d L2-normalised ArcFace embedding), both ending in ``num_tokens`` tokens of
context width behind a LayerNorm, and one ``to_k_ip`` / ``to_v_ip`` pair per cross-attention layer of the U-Net.  FaceID files also hold
rank-128 LoRA pairs for the q / k / v / out projections of every attention layer; they are kept as ``lora`` and fused into the U-Net's own
weights by ``fuse`` (``W += lora_scale * up @ down``, no alpha) through ``sd_lora``'s fuse / unfuse machinery.

The adapter is a parameter container plus the token path; the decoupled cross-attention itself runs inside the U-Net
(``UNetModel.set_ip_adapter``: one GEMM over ``packed_kv()`` at set time, ``af_ip_attention_add`` per layer and step).

Key layout (restated from tencent-ailab/IP-Adapter and diffusers; not pinned against either, no checkpoint or reference tree is at hand):
``{"image_proj": {...}, "ip_adapter": {...}}``, or flat with ``image_proj.`` / ``ip_adapter.`` prefixes (the safetensors spelling).  Keys under
``ip_adapter`` are ``"{i}.to_k_ip.weight"`` / ``"{i}.to_v_ip.weight"`` with i the index in diffusers' ``unet.attn_processors`` order (down blocks,
up blocks, mid; attn1 even, attn2 odd): ``KEY_INDEX[j]`` for the j-th layer of ``UNetModel._cross_attn_layers()`` (input, middle, output)."""
import os

import torch
import torch.nn as nn

from .. import ops
from ..ldm.modules.diffusionmodules.util import LayerNorm, Linear, _PackCache
from ..ops import F16
from . import sd_lora

# j (UNetModel._cross_attn_layers(): 6 input, 1 middle, 9 output) -> i of "{i}.to_k_ip" (diffusers' attn_processors order: down, up, mid)
KEY_INDEX = (1, 3, 5, 7, 9, 11, 31, 13, 15, 17, 19, 21, 23, 25, 27, 29)
CLIP_EMBED_DIM = 1024           # CLIPVisionModelWithProjection (ViT-H/14) image_embeds
FACE_ID_DIM = 512               # ArcFace embedding; MLPProjModel's hidden width is twice that
LORA_LEAVES = {"to_q_lora": "to_q", "to_k_lora": "to_k", "to_v_lora": "to_v", "to_out_lora": "to_out.0"}
KINDS = ("clip", "faceid")


def cross_attn_layout(unet_config):
    """[(LDM path of the SpatialTransformer, channels)] of UNetModel(**unet_config)'s cross-attention layers, in _cross_attn_layers() order."""
    mc, mult, nrb = unet_config["model_channels"], list(unet_config["channel_mult"]), unet_config["num_res_blocks"]
    ares = list(unet_config["attention_resolutions"])
    out, ds, idx = [], 1, 1
    for level, m in enumerate(mult):
        for _ in range(nrb):
            if ds in ares:
                out.append((f"input_blocks.{idx}.1", mc * m))
            idx += 1
        if level != len(mult) - 1:
            idx += 1
            ds *= 2
    out.append(("middle_block.1", mc * mult[-1]))
    idx = 0
    for level, m in list(enumerate(mult))[::-1]:
        for i in range(nrb + 1):
            if ds in ares:
                out.append((f"output_blocks.{idx}.1", mc * m))
            if level and i == nrb:
                ds //= 2
            idx += 1
    return out


class ImageProjModel(nn.Module):
    """proj Linear(1024, T * ctx) -> [B, T, ctx] -> norm LayerNorm(ctx)."""

    def __init__(self, context_dim, num_tokens, embed_dim=CLIP_EMBED_DIM):
        super().__init__()
        self.context_dim, self.num_tokens, self.embed_dim = context_dim, num_tokens, embed_dim
        self.proj = Linear(embed_dim, num_tokens * context_dim)
        self.norm = LayerNorm(context_dim)

    def hip(self, e):
        y = self.proj.hip(e)
        return self.norm.hip(y.reshape(-1, self.context_dim)).reshape(e.shape[0], self.num_tokens, self.context_dim)


class MLPProjModel(nn.Module):
    """proj.0 Linear(512, 1024) -> GELU -> proj.2 Linear(1024, T * ctx) -> [B, T, ctx] -> norm LayerNorm(ctx)."""

    def __init__(self, context_dim, num_tokens, embed_dim=FACE_ID_DIM):
        super().__init__()
        self.context_dim, self.num_tokens, self.embed_dim = context_dim, num_tokens, embed_dim
        self.proj = nn.Sequential(Linear(embed_dim, 2 * embed_dim), nn.GELU(), Linear(2 * embed_dim, num_tokens * context_dim))
        self.norm = LayerNorm(context_dim)

    def hip(self, e):
        y = self.proj[2].hip(ops.gelu(self.proj[0].hip(e)))
        return self.norm.hip(y.reshape(-1, self.context_dim)).reshape(e.shape[0], self.num_tokens, self.context_dim)


class IPAdapter(nn.Module):
    def __init__(self, unet_config, kind, num_tokens=4):
        super().__init__()
        if kind not in KINDS:
            raise ValueError(f"IPAdapter: kind must be one of {KINDS}, got {kind!r}")
        if not 1 <= num_tokens <= ops.IP_ATTN_MAX_TOKENS:
            raise ValueError(f"IPAdapter: num_tokens must be in 1 .. {ops.IP_ATTN_MAX_TOKENS}, got {num_tokens}")
        layout = cross_attn_layout(unet_config)
        if len(layout) != len(KEY_INDEX):
            raise ValueError(f"IPAdapter: the U-Net has {len(layout)} cross-attention layers, the SD-1.5 key table {len(KEY_INDEX)}")
        self.kind, self.num_tokens, self.context_dim = kind, num_tokens, unet_config["context_dim"]
        self.layout = layout
        self.to_k_ip = nn.ModuleList([Linear(self.context_dim, c, bias=False) for _, c in layout])
        self.to_v_ip = nn.ModuleList([Linear(self.context_dim, c, bias=False) for _, c in layout])
        self.image_proj = (ImageProjModel if kind == "clip" else MLPProjModel)(self.context_dim, num_tokens)
        self.lora = {}                  # faceid: {LDM path of a Linear: (down [r, Cin], up [Cout, r], None)}, sd_lora.fuse_unet_lora's input
        self._fused = None              # (the U-Net the LoRA is fused into, its saved originals)
        self._kv_cache = _PackCache()

    @property
    def embed_dim(self):
        return self.image_proj.embed_dim

    def packed_kv(self):
        """[all to_k_ip | all to_v_ip] stacked for the one projection GEMM of UNetModel.set_ip_adapter, packed once per weight version."""
        ws = [m.weight for m in self.to_k_ip] + [m.weight for m in self.to_v_ip]
        return self._kv_cache.get(ws, lambda: ops.pack_matrix(torch.cat([w.detach() for w in ws], 0), None, ws[0].device))

    def tokens(self, embeds):
        """embeds [B, embed_dim] (image_embeds of CLIP ViT-H/14, or L2-normalised face ids) -> fp16 [B, num_tokens, context_dim] on the device."""
        if not torch.is_tensor(embeds) or embeds.dim() != 2 or embeds.shape[1] != self.embed_dim:
            raise ValueError(f"IPAdapter.tokens: expected [B, {self.embed_dim}] embeddings for kind {self.kind!r}, got "
                             f"{tuple(embeds.shape) if torch.is_tensor(embeds) else type(embeds).__name__}")
        dev = self.to_k_ip[0].weight.device
        return self.image_proj.hip(embeds.to(dev, F16).contiguous())

    def uncond_tokens(self, B):
        """image_proj(zeros), as upstream does for the unconditional half."""
        return self.tokens(torch.zeros(B, self.embed_dim))

    # ---- the FaceID LoRA lives in the U-Net's own weights while the adapter is loaded
    def fuse(self, model, lora_scale=1.0):
        """Fuse the FaceID LoRA into ``model`` (a UNetWrapper or the UNetModel): W += lora_scale * up @ down.  No-op for kind "clip"."""
        if self._fused is not None:
            raise RuntimeError("IPAdapter.fuse: the LoRA is already fused; unfuse() first")
        if self.lora:
            self._fused = (model, sd_lora.fuse_unet_lora(model, self.lora, lora_scale))

    def unfuse(self):
        """Restore the U-Net weights saved by fuse (bit-exact)."""
        if self._fused is not None:
            model, saved = self._fused
            sd_lora.unfuse_unet_lora(model, saved)
            self._fused = None


def _lora_paths(layout):
    """{"{i}.{leaf}_lora": LDM path of the Linear} for all i in 0 .. 2 len(layout) - 1: i = KEY_INDEX[j] is attn2 of layer j, i - 1 its attn1."""
    out = {}
    for (prefix, _), i in zip(layout, KEY_INDEX):
        for ii, attn in ((i - 1, "attn1"), (i, "attn2")):
            for leaf, lin in LORA_LEAVES.items():
                out[f"{ii}.{leaf}"] = f"{prefix}.transformer_blocks.0.{attn}.{lin}"
    return out


def expected_shapes(unet_config, kind, num_tokens=4, lora_rank=128):
    """{"image_proj.<key>" | "ip_adapter.<key>": shape} of a file of this kind for this U-Net (FaceID: with its rank-``lora_rank`` LoRA pairs)."""
    ctx, layout = unet_config["context_dim"], cross_attn_layout(unet_config)
    s = {}
    if kind == "clip":
        s["image_proj.proj.weight"], s["image_proj.proj.bias"] = (num_tokens * ctx, CLIP_EMBED_DIM), (num_tokens * ctx,)
    else:
        s["image_proj.proj.0.weight"], s["image_proj.proj.0.bias"] = (2 * FACE_ID_DIM, FACE_ID_DIM), (2 * FACE_ID_DIM,)
        s["image_proj.proj.2.weight"], s["image_proj.proj.2.bias"] = (num_tokens * ctx, 2 * FACE_ID_DIM), (num_tokens * ctx,)
    s["image_proj.norm.weight"], s["image_proj.norm.bias"] = (ctx,), (ctx,)
    for (_, c), i in zip(layout, KEY_INDEX):
        s[f"ip_adapter.{i}.to_k_ip.weight"], s[f"ip_adapter.{i}.to_v_ip.weight"] = (c, ctx), (c, ctx)
        if kind == "faceid":
            for ii, cin_kv in ((i - 1, c), (i, ctx)):
                for leaf in LORA_LEAVES:
                    cin = cin_kv if leaf in ("to_k_lora", "to_v_lora") else c
                    s[f"ip_adapter.{ii}.{leaf}.down.weight"], s[f"ip_adapter.{ii}.{leaf}.up.weight"] = (lora_rank, cin), (c, lora_rank)
    return s


def _flatten(sd):
    """Both container spellings -> {"image_proj.<key>" | "ip_adapter.<key>": tensor}."""
    if isinstance(sd.get("image_proj"), dict) or isinstance(sd.get("ip_adapter"), dict):
        extra = [k for k in sd if k not in ("image_proj", "ip_adapter")]
        if extra or not isinstance(sd.get("image_proj"), dict) or not isinstance(sd.get("ip_adapter"), dict):
            raise ValueError(f"an IP-Adapter file holds exactly the dicts 'image_proj' and 'ip_adapter', got {sorted(map(str, sd))}")
        return {f"{part}.{k}": v for part in ("image_proj", "ip_adapter") for k, v in sd[part].items()}
    return dict(sd)


def load_ip_adapter(path_or_state_dict, unet_config, num_tokens=4):
    """An IPAdapter from a published file (``.bin`` with two dicts, or ``.safetensors`` with prefixes) or such a state dict, strictly: every
    missing, unexpected or mis-shaped key is named.  The kind is read from the keys.  Refused by name: the Plus / Resampler variants
    (``image_proj.latents`` / ``image_proj.layers.*``), an SDXL file (2048-wide tokens), a file whose two parts are of different kinds."""
    sd = sd_lora.load_lora_file(path_or_state_dict) if isinstance(path_or_state_dict, (str, os.PathLike)) else path_or_state_dict
    flat = _flatten(sd)
    if any(k == "image_proj.latents" or k.startswith(("image_proj.layers.", "image_proj.proj_in.", "image_proj.proj_out.")) for k in flat):
        raise ValueError("this is an IP-Adapter Plus file (image_proj is a Resampler: latents / layers.*): the Plus variants are not built")
    has_mlp, has_lin = "image_proj.proj.0.weight" in flat, "image_proj.proj.weight" in flat
    has_lora = any("_lora." in k for k in flat)
    if has_mlp == has_lin:
        raise ValueError("image_proj holds neither 'proj.weight' (kind 'clip') nor 'proj.0.weight' (kind 'faceid'), or both")
    kind = "faceid" if has_mlp else "clip"
    if has_lora != has_mlp:
        raise ValueError(f"kind mismatch: image_proj is of kind {kind!r} but ip_adapter holds {'' if has_lora else 'no '}FaceID LoRA keys")
    ctx = unet_config["context_dim"]
    for k, v in flat.items():
        if k.endswith(".to_k_ip.weight") and v.dim() == 2 and v.shape[1] == 2048 and ctx != 2048:
            raise ValueError(f"this is an SDXL IP-Adapter ({k} reads 2048-wide tokens, the U-Net's context is {ctx}): SDXL is not built")
    rank = next((v.shape[0] for k, v in flat.items() if k.endswith("_lora.down.weight") and v.dim() == 2), 128)
    want = expected_shapes(unet_config, kind, num_tokens, rank)
    missing = sorted(set(want) - set(flat))
    extra = sorted(set(flat) - set(want))
    bad = [f"{k}: {tuple(flat[k].shape)}, want {want[k]}" for k in sorted(want) if k in flat and tuple(flat[k].shape) != tuple(want[k])]
    if missing or extra or bad:
        raise ValueError(f"IP-Adapter ({kind}) state dict does not fit this U-Net: missing {missing}; unexpected {extra}; mis-shaped {bad}")
    ad = IPAdapter(unet_config, kind, num_tokens)
    ad.image_proj.load_state_dict({k[len("image_proj."):]: v for k, v in flat.items() if k.startswith("image_proj.")}, strict=True)
    for j, i in enumerate(KEY_INDEX):
        with torch.no_grad():
            ad.to_k_ip[j].weight.copy_(flat[f"ip_adapter.{i}.to_k_ip.weight"])
            ad.to_v_ip[j].weight.copy_(flat[f"ip_adapter.{i}.to_v_ip.weight"])
    if kind == "faceid":
        ad.lora = {path: (flat[f"ip_adapter.{key}.down.weight"], flat[f"ip_adapter.{key}.up.weight"], None)
                   for key, path in _lora_paths(ad.layout).items()}
    return ad.eval()
