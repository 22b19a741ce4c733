"""ControlNet for the SD-1.5 U-Net: a restatement of ``cldm.ControlNet`` (lllyasviel/ControlNet, ``cldm/cldm.py``) with the published parameter
names -- ``time_embed.{0,2}``, ``input_blocks.*``, ``middle_block.*``, ``input_hint_block.{0,2,..,14}``, ``zero_convs.{0..11}.0`` and
``middle_block_out.0`` -- built from the classes the U-Net is built from, so its trunk runs on the tuned kernels unchanged.

What differs from the reference's op-by-op torch:

* the hint encoder (``hint_features``; eight 3x3 convolutions 3 -> 16 -> 16 -> 32 s2 -> 32 -> 96 s2 -> 96 -> 256 s2 -> model_channels on the
  full-resolution control image) runs ONCE per generation, not per step: seven launches of ``af_hint_conv3x3`` (the first reads the uint8
  image directly) and the last convolution on the tuned ``conv3x3``;
* ``conv_in`` adds the hint features in its epilogue (``residual=``);
* each of the thirteen "zero convolution, then add into the U-Net" joins is ONE GEMM whose epilogue adds the U-Net's tensor and leaves the
  GroupNorm partial statistics of the sum: ``skip + scale * (W h + b)`` goes to a fresh tensor, ``scale`` folded into the packed weights;
* the time-embedding projections of its ResBlocks are one GEMM and the K / V projections of the context another, through the U-Net's own
  ``_embed`` / ``_packed_emb_all`` / ``_project_context_all``.

``UNetModel.set_control`` places it on a U-Net; ``load_controlnet`` reads a cldm-layout file.  The diffusers layout is not read."""
import torch
import torch.nn as nn

from .... import SD15_UNET_CONFIG, ops
from ..attention import SpatialTransformer
from .openaimodel import Downsample, ResBlock, TimestepEmbedSequential, UNetModel
from .util import _PackCache, conv_nd, linear, zero_module

HINT_WIDTHS = ((16, 1), (16, 1), (32, 2), (32, 1), (96, 2), (96, 1), (256, 2))     # (cout, stride) of input_hint_block.{0,2,..,12}; .14: 256 -> model_channels


class ControlNet(nn.Module):
    """``cldm.ControlNet`` for the options SD-1.5 uses (the U-Net's constructor arguments; ``out_channels`` and the decoder-only ones are
    accepted and ignored, so ``ControlNet(**unet_config)`` builds the ControlNet of that U-Net)."""

    def __init__(self, in_channels, model_channels, num_res_blocks, attention_resolutions, hint_channels=3, dropout=0, channel_mult=(1, 2, 4, 8),
                 conv_resample=True, dims=2, use_checkpoint=False, num_heads=-1, num_head_channels=-1, use_spatial_transformer=False,
                 transformer_depth=1, context_dim=None, out_channels=None, use_fp16=False, num_heads_upsample=-1, legacy=True, **unused):
        super().__init__()
        if not use_spatial_transformer or context_dim is None or dims != 2:
            raise NotImplementedError("only the use_spatial_transformer=True / context_dim path (SD-1.x) is implemented")
        if hint_channels != 3:
            raise NotImplementedError("the hint encoder reads RGB control images (hint_channels = 3)")
        if isinstance(context_dim, (list, tuple)) or type(context_dim).__name__ == "ListConfig":
            context_dim = list(context_dim)[0]
        if num_heads == -1 and num_head_channels == -1:
            raise ValueError("Either num_heads or num_head_channels has to be set")
        self.in_channels, self.model_channels, self.num_res_blocks = in_channels, model_channels, num_res_blocks
        self.attention_resolutions, self.channel_mult = attention_resolutions, channel_mult
        self.num_heads, self.num_head_channels, self.context_dim = num_heads, num_head_channels, context_dim

        def transformer(ch):
            n, d = (num_heads, ch // num_heads) if num_head_channels == -1 else (ch // num_head_channels, num_head_channels)
            return SpatialTransformer(ch, n, d, depth=transformer_depth, context_dim=context_dim)

        def zero_conv(ch):
            return TimestepEmbedSequential(zero_module(conv_nd(dims, ch, ch, 1, padding=0)))

        time_embed_dim = model_channels * 4
        self.time_embed = nn.Sequential(linear(model_channels, time_embed_dim), nn.SiLU(), linear(time_embed_dim, time_embed_dim))
        conv_in = conv_nd(dims, in_channels, model_channels, 3, padding=1)
        conv_in.cin_pad = ops.round_up(in_channels, 8)
        self.input_blocks = nn.ModuleList([TimestepEmbedSequential(conv_in)])
        self.zero_convs = nn.ModuleList([zero_conv(model_channels)])
        hint, cin = [], hint_channels
        for cout, stride in HINT_WIDTHS:
            hint += [conv_nd(dims, cin, cout, 3, padding=1, stride=stride), nn.SiLU()]
            cin = cout
        self.input_hint_block = TimestepEmbedSequential(*hint, zero_module(conv_nd(dims, cin, model_channels, 3, padding=1)))
        ch, ds = model_channels, 1
        for level, mult in enumerate(channel_mult):
            for _ in range(num_res_blocks):
                layers = [ResBlock(ch, time_embed_dim, dropout, out_channels=mult * model_channels, dims=dims, use_checkpoint=use_checkpoint)]
                ch = mult * model_channels
                if ds in attention_resolutions:
                    layers.append(transformer(ch))
                self.input_blocks.append(TimestepEmbedSequential(*layers))
                self.zero_convs.append(zero_conv(ch))
            if level != len(channel_mult) - 1:
                self.input_blocks.append(TimestepEmbedSequential(Downsample(ch, conv_resample, dims=dims, out_channels=ch)))
                self.zero_convs.append(zero_conv(ch))
                ds *= 2
        self.middle_block = TimestepEmbedSequential(
            ResBlock(ch, time_embed_dim, dropout, dims=dims, use_checkpoint=use_checkpoint),
            transformer(ch),
            ResBlock(ch, time_embed_dim, dropout, dims=dims, use_checkpoint=use_checkpoint),
        )
        self.middle_block_out = zero_conv(ch)
        self._assign_emb_slices()
        self._hint_caches = [_PackCache() for _ in HINT_WIDTHS]
        self._zero_caches = [_PackCache() for _ in range(len(self.zero_convs) + 1)]
        self._zero_scale = None
        self.eval().requires_grad_(False)

    # the one-GEMM time-embedding and K / V projections are the U-Net's own functions, run on this module's layers (it has no decoder)
    output_blocks = ()
    _assign_emb_slices = UNetModel._assign_emb_slices
    _packed_emb_all = UNetModel._packed_emb_all
    _embed = UNetModel._embed
    _cross_attn_layers = UNetModel._cross_attn_layers
    _project_context_all = UNetModel._project_context_all

    # ------------------------------------------------------------------ hint encoder (once per generation)
    def _packed_hint(self, k):
        conv = self.input_hint_block[2 * k]
        if not conv.weight.is_cuda:
            raise RuntimeError(f"ControlNet: parameters are on {conv.weight.device}; the hint encoder only runs on an MI355X (HIP extension, "
                               "no CPU fallback). Move the module with .cuda() first.")
        return self._hint_caches[k].get((conv.weight, conv.bias),
                                        lambda: (ops.pack_hint_conv3x3(conv.weight), conv.bias.detach().float().contiguous()))

    def hint_features(self, images_u8):
        """uint8 RGB control images [B0, 8h, 8w, 3] on the device -> fp16 [B0, h, w, model_channels]."""
        x = images_u8
        if not torch.is_tensor(x) or x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3 or x.shape[1] % 8 or x.shape[2] % 8 or x.numel() == 0:
            raise ValueError("hint_features: control images must be uint8 [B0, 8h, 8w, 3], got "
                             f"{(x.dtype, tuple(x.shape)) if torch.is_tensor(x) else type(x).__name__}")
        x = x.contiguous()
        for k, (_, stride) in enumerate(HINT_WIDTHS):
            wt, bias = self._packed_hint(k)
            x = ops.hint_conv3x3(x, wt, bias, stride=stride, act=True)
        return self.input_hint_block[2 * len(HINT_WIDTHS)].hip(x)

    # ------------------------------------------------------------------ the thirteen joins
    def _packed_zero(self, i, scale):
        """Zero convolution i (12: middle_block_out) as a GEMM weight with ``scale`` folded into weight and bias; all thirteen are repacked
        when the scale changes."""
        if scale != self._zero_scale:
            self._zero_caches = [_PackCache() for _ in self._zero_caches]
            self._zero_scale = scale
        conv = (self.zero_convs[i] if i < len(self.zero_convs) else self.middle_block_out)[0]
        return self._zero_caches[i].get((conv.weight, conv.bias), lambda: ops.pack_matrix(
            conv.weight.detach().float().reshape(conv.out_channels, conv.in_channels) * scale, conv.bias.detach().float() * scale, conv.weight.device))

    def _join(self, i, h, base, scale):
        """base + scale * zero_conv_i(h) as ONE GEMM into a fresh tensor that carries the GroupNorm partial statistics of the sum (ops.partials_of):
        ``base``, whose own statistics the decoder must no longer trust, is never written."""
        B, H, W, C = h.shape
        if tuple(base.shape) != tuple(h.shape):
            raise ValueError(f"ControlNet: residual {i} is {tuple(h.shape)}, the U-Net's tensor {tuple(base.shape)}")
        out = ops.gemm(h.reshape(B * H * W, C), self._packed_zero(i, scale), residual=base.reshape(B * H * W, C), rows_per_batch=H * W,
                       gn_cpg=C // 32 if C % 32 == 0 else 0)
        out4 = out.reshape(B, H, W, C)
        if hasattr(out, "_gn_partials"):
            out4._gn_partials = out._gn_partials      # a view: same storage address and version counter (ops.partials_of)
        return out4

    def join_middle(self, mid, unet_mid, scale):
        return self._join(len(self.zero_convs), mid, unet_mid, scale)

    # ------------------------------------------------------------------ per-step walk
    def hip_walk(self, x_nhwc, timesteps, context, hint, skips, scale=1.0, img_mask=None):
        """x_nhwc [B,H,W,8] fp16, timesteps [B], context [B,L,ctx] fp16, hint [B,H,W,model_channels] fp16 (hint_features, expanded to the batch),
        skips: the U-Net's twelve input-block outputs -> ([skip_i + scale * zero_conv_i(h_i)], h_mid): fresh skip tensors and this network's
        middle-block output, which ``join_middle`` adds to the U-Net's once that exists."""
        if len(skips) != len(self.input_blocks):
            raise ValueError(f"ControlNet: {len(skips)} skip tensors for {len(self.input_blocks)} input blocks")
        emb = self._embed(timesteps)
        kv_layers = self._project_context_all(context)
        try:
            joined = []
            h = self.input_blocks[0][0].hip(x_nhwc, residual=hint)
            joined.append(self._join(0, h, skips[0], scale))
            for i in range(1, len(self.input_blocks)):
                h = self.input_blocks[i].hip(h, emb, context, img_mask)
                joined.append(self._join(i, h, skips[i], scale))
            return joined, self.middle_block.hip(h, emb, context, img_mask)
        finally:
            for m in kv_layers:
                m._kv_pre = None


def _read_state_dict(src):
    if isinstance(src, dict):
        return src
    path = str(src)
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        sd = load_file(path)
    else:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and isinstance(sd.get("state_dict"), dict):
        sd = sd["state_dict"]
    return sd


def load_controlnet(path_or_state_dict, unet_config=SD15_UNET_CONFIG):
    """A ControlNet for the U-Net of ``unet_config`` from a cldm-layout ``.pth`` / ``.ckpt`` / ``.safetensors`` file or state dict.  Keys are
    bare or carry the ``control_model.`` prefix; if any key carries it only those are read (a v1.0 file also holds the whole SD-1.5 model).
    Strict: a missing, unexpected or mis-shaped key raises ValueError naming it.  A diffusers-layout file is refused.  Nothing is downloaded."""
    sd = _read_state_dict(path_or_state_dict)
    if any(k.startswith(("controlnet_cond_embedding.", "controlnet_down_blocks.", "controlnet_mid_block.")) for k in sd):
        raise ValueError("load_controlnet: this is the diffusers ControlNetModel layout (controlnet_cond_embedding.* / controlnet_down_blocks.*), "
                         "which is not read: pass the cldm-layout file (control_model.* keys, e.g. control_v11p_sd15_openpose.pth)")
    prefix = "control_model."
    if any(k.startswith(prefix) for k in sd):
        sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    net = ControlNet(**unet_config)
    own = net.state_dict()
    missing = sorted(k for k in own if k not in sd)
    unexpected = sorted(k for k in sd if k not in own)
    misshaped = [f"{k} {tuple(sd[k].shape)} (expected {tuple(v.shape)})" for k, v in own.items()
                 if k in sd and (not torch.is_tensor(sd[k]) or tuple(sd[k].shape) != tuple(v.shape))]
    if missing or unexpected or misshaped:
        raise ValueError("ControlNet state dict does not match"
                         + (f"; missing: {missing}" if missing else "")
                         + (f"; unexpected: {unexpected}" if unexpected else "")
                         + (f"; wrong shape: {misshaped}" if misshaped else ""))
    net.load_state_dict({k: sd[k].float() for k in own}, strict=True)
    return net


def guidance_window_active(i, n, start=0.0, end=1.0):
    """diffusers' control_guidance_start / control_guidance_end rule: control is on at step i of n iff i / n >= start and (i + 1) / n <= end."""
    return i / n >= start and (i + 1) / n <= end
