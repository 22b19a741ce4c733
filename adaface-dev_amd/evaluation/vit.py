"""The encoders the reference scores its outputs with (``evaluation/clip_eval.py``, ``evaluation/eval_utils.py``): the CLIP vision and text
towers (``clip.load("ViT-B/32")``) and the DINO ViT-S/16 (``ViTModel.from_pretrained("facebook/dino-vits16")``), executed with this package's
gfx950 kernels.  The reference tree is not available here: the contract is restated from openai/CLIP (``clip/model.py``), ``transformers``
(``CLIPVisionModelWithProjection``, ``CLIPTextModelWithProjection``, ``ViTModel``) and torchvision's ``Resize`` / ``CenterCrop`` /
``Normalize`` -- INTEGRATION.md "Scoring images".

``VisionTransformer.forward_u8`` takes uint8 images of any size on the device:

    af_vit_patch_rows (resize + crop + normalise + unfold, one launch) -> patch GEMM -> [CLS | patches] + positions -> (pre-LN) ->
    ``CLIPEncoderLayer`` x L (fused q|k|v GEMM, ``af_attention`` without the causal mask, quick-GELU epilogue or ``af_gelu_f16``) -> head.

The trunk is the layer class the text encoders run on (``adaface/arc2face_models.py``); ``patch_mask`` is the mechanism of the reference's
``CLIPVisionModelWithMask`` (``adaface/util.py:321-414``): a key bias of 0 / -FLT_MAX on the patch tokens in every layer, CLS always visible."""
import os
import re
from types import SimpleNamespace

import torch
import torch.nn as nn

from .. import ops
from ..adaface.arc2face_models import CLIPEncoderLayer, CLIPTextModelWrapper, clip_text_config
from ..ldm.modules.diffusionmodules.util import LayerNorm, Linear, _PackCache
from ..ops import F16

CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

_CLIP_VISION = {"ViT-B/32": dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, patch_size=32, projection_dim=512),
                "ViT-L/14": dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, patch_size=14, projection_dim=768),
                # OpenCLIP's ViT-H/14 as transformers ships it (laion/CLIP-ViT-H-14-laion2B-s32B-b79K, IP-Adapter's image encoder): 80-wide heads, erf-GELU
                "ViT-H/14": dict(hidden_size=1280, num_hidden_layers=32, num_attention_heads=16, patch_size=14, projection_dim=1024,
                                 intermediate_size=5120, hidden_act="gelu")}
# the text tower that goes with each vision tower (openai/CLIP's model table)
_CLIP_TEXT = {"ViT-B/32": dict(hidden_size=512, num_attention_heads=8, num_hidden_layers=12, intermediate_size=2048),
              "ViT-L/14": dict(hidden_size=768, num_attention_heads=12, num_hidden_layers=12, intermediate_size=3072)}


def _vit_config(**kw):
    c = SimpleNamespace(**dict(dict(image_size=224, attention_dropout=0.0), **kw))
    if not getattr(c, "intermediate_size", 0):
        c.intermediate_size = 4 * c.hidden_size
    return c


def clip_vision_config(name="ViT-B/32", **overrides):
    """CLIP's vision tower: pre-LN ("pre_layrnorm", transformers' spelling), quick-GELU, eps 1e-5, patch convolution without bias, CLS ->
    post_layernorm -> projection without bias.  CLIP preprocess: Resize(224) bicubic, CenterCrop(224), CLIP mean / std."""
    if name not in _CLIP_VISION:
        raise ValueError(f"clip_vision_config: unknown model {name!r} (known: {sorted(_CLIP_VISION)})")
    kw = dict(hidden_act="quick_gelu", layer_norm_eps=1e-5, pre_layernorm=True, patch_bias=False, pool="cls_post_ln",
              keep_aspect=True, filter="bicubic", mean=CLIP_MEAN, std=CLIP_STD)
    kw.update(_CLIP_VISION[name])
    kw.update(overrides)
    return _vit_config(**kw)


def dino_vit_config(**overrides):
    """facebook/dino-vits16 (ViT-S/16): erf-GELU, eps 1e-12, patch convolution with bias, no pre-LN, no projection, the final LayerNorm over
    all tokens and its CLS row as the feature.  HF ViT feature extractor: square bilinear resize to 224, ImageNet mean / std."""
    kw = dict(hidden_size=384, num_hidden_layers=12, num_attention_heads=6, patch_size=16, projection_dim=0, hidden_act="gelu",
              layer_norm_eps=1e-12, pre_layernorm=False, patch_bias=True, pool="ln_cls", keep_aspect=False, filter="bilinear",
              mean=IMAGENET_MEAN, std=IMAGENET_STD)
    kw.update(overrides)
    return _vit_config(**kw)


def clip_text_tower_config(name="ViT-B/32", projection_dim=None, **overrides):
    kw = dict(_CLIP_TEXT[name], eos_token_id=49407)
    kw.update(overrides)
    c = clip_text_config(**kw)
    c.projection_dim = projection_dim or _CLIP_VISION[name]["projection_dim"]
    return c


class VisionTransformer(nn.Module):
    """Parameter names: ``class_embedding`` [E], ``patch_embedding.weight`` [E, 3, p, p] (``.bias``), ``position_embedding`` [P + 1, E],
    ``pre_layrnorm``, ``layers.N`` (``CLIPEncoderLayer``), ``post_layernorm``, ``visual_projection.weight`` [D, E]."""

    def __init__(self, config=None):
        super().__init__()
        c = self.config = config or clip_vision_config()
        E, p = c.hidden_size, c.patch_size
        if c.image_size % p or E % c.num_attention_heads:
            raise ValueError(f"VisionTransformer: image {c.image_size} / patch {p} or width {E} / heads {c.num_attention_heads} do not divide")
        if c.pool not in ("cls_post_ln", "ln_cls"):
            raise ValueError(f"VisionTransformer: pool must be 'cls_post_ln' or 'ln_cls', got {c.pool!r}")
        self.num_patches = (c.image_size // p) ** 2
        self.class_embedding = nn.Parameter(torch.zeros(E))
        self.patch_embedding = nn.Conv2d(3, E, p, stride=p, bias=bool(c.patch_bias))       # a parameter holder: executed as a GEMM
        self.position_embedding = nn.Parameter(torch.zeros(self.num_patches + 1, E))
        self.pre_layrnorm = LayerNorm(E, eps=c.layer_norm_eps) if c.pre_layernorm else None
        self.layers = nn.ModuleList([CLIPEncoderLayer(c) for _ in range(c.num_hidden_layers)])
        self.post_layernorm = LayerNorm(E, eps=c.layer_norm_eps)
        self.visual_projection = Linear(E, c.projection_dim, bias=False) if c.projection_dim else None
        self._patch_cache = _PackCache()

    @property
    def feature_dim(self):
        return self.config.projection_dim or self.config.hidden_size

    def patch_kcols(self):
        return ops.round_up(3 * self.config.patch_size ** 2, 64)

    def _patch_packed(self):
        w, b = self.patch_embedding.weight, self.patch_embedding.bias
        if not w.is_cuda:
            raise RuntimeError("VisionTransformer: parameters are on the CPU; this model only runs on an MI355X (HIP extension, no CPU "
                               "fallback). Move it with .cuda() first.")

        def build():
            E, k = w.shape[0], 3 * self.config.patch_size ** 2
            m = torch.zeros((E, self.patch_kcols()), device=w.device)         # columns 3 p^2 .. meet the zeros af_vit_patch_rows writes
            m[:, :k] = w.detach().float().reshape(E, k)
            return ops.pack_matrix(m, b, w.device)
        return self._patch_cache.get((w, b), build)

    def patch_rows(self, images_u8):
        c = self.config
        return ops.vit_patch_rows(images_u8, keep_aspect=c.keep_aspect, S=c.image_size, C=c.image_size, p=c.patch_size, filter=c.filter,
                                  mean=c.mean, std=c.std, kpad=self.patch_kcols())

    @torch.no_grad()
    def forward_rows(self, rows, B, patch_mask=None):
        """rows fp16 [B * P, patch_kcols()] -> (transformers' ``last_hidden_state`` fp16 [B, P + 1, E]: the encoder output for CLIP, the
        final LayerNorm of it for DINO; features fp16 [B, feature_dim])."""
        c, P, E = self.config, self.num_patches, self.config.hidden_size
        T = P + 1
        x = ops.gemm(rows, self._patch_packed()).reshape(B, P, E)
        h = torch.empty((B, T, E), dtype=F16, device=x.device)
        pos = self.position_embedding.detach().float()
        h[:, 0] = (self.class_embedding.detach().float() + pos[0]).to(F16)
        h[:, 1:] = (x.float() + pos[1:]).to(F16)
        h = h.reshape(B * T, E)
        if self.pre_layrnorm is not None:
            h = self.pre_layrnorm.hip(h)
        keybias = None
        if patch_mask is not None:
            if patch_mask.dtype != torch.bool or tuple(patch_mask.shape) != (B, P):
                raise ValueError(f"patch_mask must be bool [{B}, {P}], got {patch_mask.dtype} {tuple(patch_mask.shape)}")
            keep = torch.cat([torch.ones((B, 1), dtype=torch.bool, device=h.device), patch_mask.to(h.device)], dim=1)     # CLS always visible
            keybias = ops.make_keybias(keep, T)
        for layer in self.layers:
            h = layer.hip(h, B, T, causal=False, keybias=keybias)
        if c.pool == "ln_cls":
            last = self.post_layernorm.hip(h).reshape(B, T, E)
            cls = last[:, 0].contiguous()
        else:
            last = h.reshape(B, T, E)
            cls = self.post_layernorm.hip(last[:, 0].contiguous())
        feats = self.visual_projection.hip(cls) if self.visual_projection is not None else cls
        return last, feats

    def forward_u8(self, images_u8, patch_mask=None, return_hidden=False):
        """uint8 [B, H, W, 3] device images of any size -> features fp16 [B, feature_dim] (and the last hidden state with return_hidden)."""
        last, feats = self.forward_rows(self.patch_rows(images_u8), images_u8.shape[0], patch_mask)
        return (feats, last) if return_hidden else feats

    forward = forward_u8


class CLIPTextTower(CLIPTextModelWrapper):
    """``CLIPTextModelWrapper`` at a CLIP model's text width + ``text_projection`` (no bias) on the pooled EOS state: transformers'
    ``CLIPTextModelWithProjection`` (keys ``text_model.*``, ``text_projection.weight``)."""

    def __init__(self, config=None):
        config = config or clip_text_tower_config()
        super().__init__(config)
        self.text_projection = Linear(config.hidden_size, config.projection_dim, bias=False)

    @torch.no_grad()
    def encode(self, input_ids, return_hidden=False):
        """token ids [B, T] -> text features fp16 [B, projection_dim] (and the last hidden state [B, T, E])."""
        out = super().forward(input_ids=input_ids.to(self.text_projection.weight.device))
        last, pooled = out[0], out[1]
        feats = self.text_projection.hip(pooled.to(F16).contiguous())
        return (feats, last) if return_hidden else feats


# ---------------------------------------------------------------------------------------------------------------------------- loaders
def _read_file(path):
    path = str(path)
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    try:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    except Exception:
        # openai's published ViT-B-32.pt is a TorchScript archive, which weights_only refuses
        sd = torch.jit.load(path, map_location="cpu").state_dict()
    for key in ("state_dict", "teacher", "model"):
        if isinstance(sd, dict) and isinstance(sd.get(key), dict):
            sd = sd[key]
    return sd


def _read_state_dict(src, what):
    sd = src if isinstance(src, dict) else _read_file(src)
    if not isinstance(sd, dict) or not all(isinstance(k, str) for k in sd):
        raise ValueError(f"{what}: expected a state dict (or a file holding one), got {type(sd).__name__}")
    return {k: v for k, v in sd.items() if torch.is_tensor(v)}


def _strict_load(module, sd, what):
    own = module.state_dict()
    missing = sorted(k for k in own if k not in sd)
    unexpected = sorted(k for k in sd if k not in own)
    misshaped = [f"{k} {tuple(sd[k].shape)} (expected {tuple(v.shape)})" for k, v in own.items() if k in sd and tuple(sd[k].shape) != tuple(v.shape)]
    if missing or unexpected or misshaped:
        raise ValueError(f"{what}: state dict does not match"
                         + (f"; missing: {missing}" if missing else "")
                         + (f"; unexpected: {unexpected}" if unexpected else "")
                         + (f"; wrong shape: {misshaped}" if misshaped else ""))
    module.load_state_dict({k: sd[k].float() for k in own}, strict=True)
    return module


def _need(sd, key, what):
    if key not in sd:
        raise ValueError(f"{what}: state dict does not match; missing: ['{key}']")
    return sd[key]


def _count(sd, pattern):
    idx = {int(m.group(1)) for k in sd for m in [re.match(pattern, k)] if m}
    return max(idx) + 1 if idx else 0


_LAYER_RENAMES_OPENAI = (("ln_1.", "layer_norm1."), ("ln_2.", "layer_norm2."), ("attn.out_proj.", "self_attn.out_proj."),
                         ("mlp.c_fc.", "mlp.fc1."), ("mlp.c_proj.", "mlp.fc2."))


def _split_qkv(out, dst, src_key, t):
    """A fused [3E, ...] q|k|v tensor -> the three projections."""
    if t.shape[0] % 3:
        raise ValueError(f"state dict does not match; wrong shape: ['{src_key} {tuple(t.shape)} (first dimension is not 3 x width)']")
    suffix = "weight" if src_key.endswith("weight") else "bias"
    for name, part in zip(("q_proj", "k_proj", "v_proj"), t.chunk(3, dim=0)):
        out[f"{dst}self_attn.{name}.{suffix}"] = part


def _openai_resblocks(sd, src_prefix, dst_prefix, out):
    """visual.transformer.resblocks.N.* / transformer.resblocks.N.* -> <dst_prefix>N.* in the CLIPEncoderLayer names; unknown keys pass through."""
    for k, v in sd.items():
        if not k.startswith(src_prefix):
            continue
        rest = k[len(src_prefix):]
        n, _, tail = rest.partition(".")
        dst = f"{dst_prefix}{n}."
        if tail in ("attn.in_proj_weight", "attn.in_proj_bias"):
            _split_qkv(out, dst, k, v)
            continue
        for a, b in _LAYER_RENAMES_OPENAI:
            if tail.startswith(a):
                tail = b + tail[len(a):]
                break
        out[dst + tail] = v


_OPENAI_IGNORED = ("logit_scale", "input_resolution", "context_length", "vocab_size")


def _clip_openai_to_hf(sd):
    """openai/CLIP's layout -> transformers' (the two tower prefixes ``vision_model.`` / ``text_model.`` and the projections)."""
    out = {}
    simple = {"visual.class_embedding": "vision_model.embeddings.class_embedding",
              "visual.positional_embedding": "vision_model.embeddings.position_embedding.weight",
              "visual.conv1.weight": "vision_model.embeddings.patch_embedding.weight",
              "visual.ln_pre.weight": "vision_model.pre_layrnorm.weight", "visual.ln_pre.bias": "vision_model.pre_layrnorm.bias",
              "visual.ln_post.weight": "vision_model.post_layernorm.weight", "visual.ln_post.bias": "vision_model.post_layernorm.bias",
              "positional_embedding": "text_model.embeddings.position_embedding.weight",
              "token_embedding.weight": "text_model.embeddings.token_embedding.weight",
              "ln_final.weight": "text_model.final_layer_norm.weight", "ln_final.bias": "text_model.final_layer_norm.bias"}
    for k, v in sd.items():
        if k in _OPENAI_IGNORED or k.startswith(("visual.transformer.resblocks.", "transformer.resblocks.")):
            continue
        if k == "visual.proj":
            out["visual_projection.weight"] = v.t()                 # stored [E, D]: x @ proj
        elif k == "text_projection":
            out["text_projection.weight"] = v.t()
        else:
            out[simple.get(k, k)] = v                                   # an unknown key stays and is reported by name
    _openai_resblocks(sd, "visual.transformer.resblocks.", "vision_model.encoder.layers.", out)
    _openai_resblocks(sd, "transformer.resblocks.", "text_model.encoder.layers.", out)
    return out


def _clip_vision_from_hf(sd, what):
    """transformers' vision keys -> this module's (and the config read from the tensors)."""
    pre = "vision_model."
    ren = {pre + "embeddings.class_embedding": "class_embedding", pre + "embeddings.position_embedding.weight": "position_embedding",
           pre + "embeddings.patch_embedding.weight": "patch_embedding.weight"}
    out = {}
    for k, v in sd.items():
        if k in ren:
            out[ren[k]] = v
        elif k.startswith(pre + "encoder.layers."):
            out["layers." + k[len(pre + "encoder.layers."):]] = v
        elif k.startswith(pre):
            out[k[len(pre):]] = v
        else:
            out[k] = v
    w = _need(out, "patch_embedding.weight", what)
    pos = _need(out, "position_embedding", what)
    proj = _need(out, "visual_projection.weight", what)
    E, p = w.shape[0], w.shape[-1]
    grid = int(round((pos.shape[0] - 1) ** 0.5))
    fc1 = _need(out, "layers.0.mlp.fc1.weight", what)
    # the state dict says neither the head count nor the activation: a tower of a known width and patch takes its table entry's (ViT-H/14:
    # 16 heads of 80, erf-GELU), any other has 64-wide heads and quick-GELU as openai's CLIP towers do
    known = next((c for c in _CLIP_VISION.values() if c["hidden_size"] == E and c["patch_size"] == p), {})
    heads = known.get("num_attention_heads", max(E // 64, 1))
    cfg = clip_vision_config("ViT-B/32", hidden_size=E, num_hidden_layers=_count(out, r"layers\.(\d+)\."), num_attention_heads=heads,
                             patch_size=p, image_size=grid * p, projection_dim=proj.shape[0], intermediate_size=fc1.shape[0],
                             hidden_act=known.get("hidden_act", "quick_gelu"))
    return out, cfg


def _clip_text_from_hf(sd, what):
    tok = _need(sd, "text_model.embeddings.token_embedding.weight", what)
    pos = _need(sd, "text_model.embeddings.position_embedding.weight", what)
    proj = _need(sd, "text_projection.weight", what)
    fc1 = _need(sd, "text_model.encoder.layers.0.mlp.fc1.weight", what)
    E = tok.shape[1]
    cfg = clip_text_config(hidden_size=E, num_attention_heads=max(E // 64, 1), num_hidden_layers=_count(sd, r"text_model\.encoder\.layers\.(\d+)\."),
                           intermediate_size=fc1.shape[0], vocab_size=tok.shape[0], max_position_embeddings=pos.shape[0],
                           eos_token_id=tok.shape[0] - 1)              # CLIP's vocabulary ends with <|endoftext|> (49407 of 49408)
    cfg.projection_dim = proj.shape[0]
    return cfg


def load_clip(path_or_state_dict, vision_heads=None, text_heads=None):
    """-> (``VisionTransformer``, ``CLIPTextTower``) from a CLIP checkpoint in transformers' layout (``vision_model.*``, ``visual_projection``,
    ``text_model.*``, ``text_projection``; ``position_ids`` buffers ignored) or openai/CLIP's (``visual.*``, ``transformer.resblocks.*``,
    fused ``in_proj``, ``visual.proj`` / ``text_projection`` stored transposed; ``logit_scale`` and the scalar attributes ignored), from a
    ``.pt`` / ``.bin`` / ``.safetensors`` file or a state dict.  Widths and depths are read from the tensors; heads are 64 wide as in every
    published CLIP (``vision_heads`` / ``text_heads`` override).  Strict: a missing, unexpected or mis-shaped key raises ValueError naming
    it.  Nothing is downloaded."""
    what = "load_clip"
    sd = _read_state_dict(path_or_state_dict, what)
    if any(k.startswith("visual.") for k in sd) or "positional_embedding" in sd:
        sd = _clip_openai_to_hf(sd)
    sd = {k: v for k, v in sd.items() if not k.endswith("position_ids") and k != "logit_scale"}
    text_sd = {k: v for k, v in sd.items() if k.startswith("text_model.") or k == "text_projection.weight"}
    vis_sd, vcfg = _clip_vision_from_hf({k: v for k, v in sd.items() if k not in text_sd}, what)
    tcfg = _clip_text_from_hf(text_sd, what)
    if vision_heads:
        vcfg.num_attention_heads = vision_heads
    if text_heads:
        tcfg.num_attention_heads = text_heads
    vision = _strict_load(VisionTransformer(vcfg), vis_sd, what + " (vision tower)")
    text = _strict_load(CLIPTextTower(tcfg), text_sd, what + " (text tower)")
    return vision.eval(), text.eval()


def load_clip_vision(path_or_state_dict, heads=None):
    """-> ``VisionTransformer`` from transformers' ``CLIPVisionModelWithProjection`` layout (``vision_model.*``, ``visual_projection.weight``), e.g.
    IP-Adapter's ViT-H/14 image encoder; its feature is ``image_embeds``, the projected CLS.  Strict like ``load_clip``; nothing is downloaded."""
    what = "load_clip_vision"
    sd = {k: v for k, v in _read_state_dict(path_or_state_dict, what).items() if not k.endswith("position_ids")}
    vis_sd, vcfg = _clip_vision_from_hf(sd, what)
    if heads:
        vcfg.num_attention_heads = heads
    return _strict_load(VisionTransformer(vcfg), vis_sd, what).eval()


_DINO_FB_LAYER = (("norm1.", "layer_norm1."), ("norm2.", "layer_norm2."), ("attn.proj.", "self_attn.out_proj."), ("mlp.fc1.", "mlp.fc1."),
                  ("mlp.fc2.", "mlp.fc2."))
_DINO_HF_LAYER = (("layernorm_before.", "layer_norm1."), ("layernorm_after.", "layer_norm2."), ("attention.attention.query.", "self_attn.q_proj."),
                  ("attention.attention.key.", "self_attn.k_proj."), ("attention.attention.value.", "self_attn.v_proj."),
                  ("attention.output.dense.", "self_attn.out_proj."), ("intermediate.dense.", "mlp.fc1."), ("output.dense.", "mlp.fc2."),
                  # transformers 5 saves the same model as layers.N.attention.{q,k,v,o}_proj / mlp.fc1 / mlp.fc2
                  ("attention.q_proj.", "self_attn.q_proj."), ("attention.k_proj.", "self_attn.k_proj."), ("attention.v_proj.", "self_attn.v_proj."),
                  ("attention.o_proj.", "self_attn.out_proj."))


def _dino_to_own(sd):
    hf = any(k.startswith(("embeddings.", "encoder.layer.")) for k in sd)
    top = ({"embeddings.cls_token": "class_embedding", "embeddings.position_embeddings": "position_embedding",
            "embeddings.patch_embeddings.projection.weight": "patch_embedding.weight",
            "embeddings.patch_embeddings.projection.bias": "patch_embedding.bias", "layernorm.weight": "post_layernorm.weight",
            "layernorm.bias": "post_layernorm.bias"} if hf else
           {"cls_token": "class_embedding", "pos_embed": "position_embedding", "patch_embed.proj.weight": "patch_embedding.weight",
            "patch_embed.proj.bias": "patch_embedding.bias", "norm.weight": "post_layernorm.weight", "norm.bias": "post_layernorm.bias"})
    lpre, renames = ("encoder.layer.", _DINO_HF_LAYER) if hf else ("blocks.", _DINO_FB_LAYER)
    if hf and not any(k.startswith(lpre) for k in sd):
        lpre = "layers."                                               # transformers 5
    out = {}
    for k, v in sd.items():
        if hf and k.startswith("pooler."):
            continue
        if k in top:
            out[top[k]] = v.reshape(v.shape[-2:]) if top[k] == "position_embedding" and v.dim() == 3 else (
                v.reshape(-1) if top[k] == "class_embedding" else v)
        elif k.startswith(lpre):
            n, _, tail = k[len(lpre):].partition(".")
            dst = f"layers.{n}."
            if not hf and tail in ("attn.qkv.weight", "attn.qkv.bias"):
                _split_qkv(out, dst, k, v)
                continue
            for a, b in renames:
                if tail.startswith(a):
                    tail = b + tail[len(a):]
                    break
            out[dst + tail] = v
        else:
            out[k] = v
    return out


def load_dino(path_or_state_dict, heads=None):
    """-> ``VisionTransformer`` from a DINO ViT checkpoint in transformers' ``ViTModel`` layout (``embeddings.*``, ``encoder.layer.N.*``,
    ``layernorm``; a ``pooler.*`` is ignored) or facebookresearch/dino's (``cls_token``, ``pos_embed``, ``patch_embed.proj``, ``blocks.N.*``
    with fused ``attn.qkv``, ``norm``).  Widths and depths are read from the tensors; heads are 64 wide (``heads`` overrides).  Strict."""
    what = "load_dino"
    own = _dino_to_own(_read_state_dict(path_or_state_dict, what))
    w = _need(own, "patch_embedding.weight", what)
    pos = _need(own, "position_embedding", what)
    fc1 = _need(own, "layers.0.mlp.fc1.weight", what)
    E, p = w.shape[0], w.shape[-1]
    grid = int(round((pos.shape[0] - 1) ** 0.5))
    cfg = dino_vit_config(hidden_size=E, num_hidden_layers=_count(own, r"layers\.(\d+)\."), num_attention_heads=heads or max(E // 64, 1),
                          patch_size=p, image_size=grid * p, intermediate_size=fc1.shape[0])
    return _strict_load(VisionTransformer(cfg), own, what).eval()
