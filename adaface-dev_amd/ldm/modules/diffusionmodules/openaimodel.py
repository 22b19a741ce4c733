"""Host-side mirror of the reference's ``ldm/modules/diffusionmodules/openaimodel.py``:
``UNetModel`` / ``ResBlock`` / ``TimestepEmbedSequential`` / ``Upsample`` / ``Downsample``
with the reference constructor arguments, state-dict keys and ``forward`` contracts
(openaimodel.py:73-161, 164-276, 414-952), executed by hand-written gfx950 kernels.

Execution plan of one epsilon-prediction (what differs from the reference's op-by-op torch):

* NCHW fp32 latents are converted once to NHWC fp16 (4 -> 8 channels zero-padded for 16-byte
  loads) and back once at the end; everything in between is NHWC fp16 in HBM;
* ResBlock = GroupNorm+SiLU kernel -> conv3x3 (bias + time-embedding add in the epilogue) ->
  GroupNorm+SiLU -> conv3x3 (bias + skip add in the epilogue); the 1x1 skip conv, the nearest
  upsample (openaimodel.py:117) and the ``torch.cat([h, hs.pop()], 1)`` of the decoder
  (openaimodel.py:918) are fused into the operand loaders of the kernels that consume them;
* the 22 per-ResBlock ``emb_layers`` Linear(SiLU(emb)) (openaimodel.py:219-225,265) are one
  GEMM per forward (weights concatenated at pack time), SiLU fused into the epilogue of
  ``time_embed.2``.
"""
import os
from abc import abstractmethod

import torch
import torch.nn as nn

from .... import ops
from ....ops import AF_ACT_SILU, F16
from ..attention import SpatialTransformer
from .util import (_PackCache, checkpoint, conv_nd, from_nhwc_f16, linear, normalization, timestep_embedding,
                   to_nhwc_f16, zero_module)


class TimestepBlock(nn.Module):
    @abstractmethod
    def forward(self, x, emb):
        """Apply the module to `x` given `emb` timestep embeddings."""


# AF_FUSE_SKIP=0: the ResBlock's 1x1 skip_connection as its own launch (A/B runs); default: K-concatenated into the second convolution
FUSE_SKIP = os.environ.get("AF_FUSE_SKIP", "1") != "0"


class SkipCat(tuple):
    """(h, skip): the decoder's channel concat, kept as two tensors so consumers read both
    sources directly instead of materialising torch.cat (openaimodel.py:918)."""


class EmbPack:
    """Time embedding handed to ResBlocks inside UNetModel: SiLU(emb) plus, when available, the
    batched output of every ResBlock's emb_layers projection."""

    def __init__(self, silu_emb, all_out=None):
        self.silu_emb = silu_emb  # [B, emb_ch] fp16
        self.all_out = all_out    # [B, sum(Cout)] fp16 or None


class TimestepEmbedSequential(nn.Sequential, TimestepBlock):
    def hip(self, x, emb, context=None, mask=None):
        for layer in self:
            if isinstance(layer, TimestepBlock):
                x = layer.hip(x, emb)
            elif isinstance(layer, SpatialTransformer):
                x = layer.hip(x, context, mask)
            else:
                x = layer.hip(x)
        return x

    def hip_train(self, x, emb, context=None, mask=None):
        saved = []
        for layer in self:
            if isinstance(layer, TimestepBlock):
                x, s = layer.hip_train(x, emb)
            elif isinstance(layer, SpatialTransformer):
                x, s = layer.hip_train(x, context, mask)
            else:
                x, s = layer.hip_train(x)
            saved.append(s)
        return x, saved

    def hip_bwd(self, saved, dy, dctx=None):
        """Reverse walk; returns (dx or (dx_h, dx_skip) for a SkipCat input, dctx)."""
        for layer, s in zip(reversed(list(self)), reversed(saved)):
            if isinstance(layer, SpatialTransformer):
                dy, dctx = layer.hip_bwd(s, dy, dctx)
            else:
                dy = layer.hip_bwd(s, dy)
        return dy, dctx

    def forward(self, x, emb, context=None, mask=None):
        for layer in self:
            if isinstance(layer, TimestepBlock):
                x = layer(x, emb)
            elif isinstance(layer, SpatialTransformer):
                x = layer(x, context, mask=mask)
            else:
                x = layer(x)
        return x


class Upsample(nn.Module):
    """Nearest x2 + optional 3x3 conv; the upsample is folded into the conv's input gather."""

    def __init__(self, channels, use_conv, dims=2, out_channels=None, padding=1):
        super().__init__()
        self.channels = channels
        self.out_channels = out_channels or channels
        self.use_conv = use_conv
        self.dims = dims
        if not use_conv:
            raise NotImplementedError("Upsample(use_conv=False) is not on the SD-1.5 path")
        self.conv = conv_nd(dims, self.channels, self.out_channels, 3, padding=padding)

    def hip(self, x):
        assert x.shape[-1] == self.channels
        return self.conv.hip(x, upsample=True)

    def hip_train(self, x):
        return self.hip(x), None

    def hip_bwd(self, saved, dy):
        return self.conv.hip_dgrad(dy, upsampled=True)

    def forward(self, x):
        assert x.shape[1] == self.channels
        return from_nhwc_f16(self.hip(to_nhwc_f16(x)), x.dtype)


class Downsample(nn.Module):
    def __init__(self, channels, use_conv, dims=2, out_channels=None, padding=1):
        super().__init__()
        self.channels = channels
        self.out_channels = out_channels or channels
        self.use_conv = use_conv
        self.dims = dims
        if not use_conv:
            raise NotImplementedError("Downsample(use_conv=False) is not on the SD-1.5 path")
        self.op = conv_nd(dims, self.channels, self.out_channels, 3, stride=2, padding=padding)

    def hip(self, x):
        assert x.shape[-1] == self.channels
        return self.op.hip(x)

    def hip_train(self, x):
        return self.hip(x), (x.shape[1], x.shape[2])

    def hip_bwd(self, saved, dy):
        return self.op.hip_dgrad(dy, in_hw=saved)

    def forward(self, x):
        assert x.shape[1] == self.channels
        return from_nhwc_f16(self.hip(to_nhwc_f16(x)), x.dtype)


class ResBlock(TimestepBlock):
    def __init__(self, channels, emb_channels, dropout, out_channels=None, use_conv=False, use_scale_shift_norm=False,
                 dims=2, use_checkpoint=False, up=False, down=False):
        super().__init__()
        if use_scale_shift_norm or up or down:
            raise NotImplementedError("scale-shift norm / resblock_updown are not on the SD-1.5 path")
        if dropout != 0:
            raise NotImplementedError("dropout > 0 is not supported (SD-1.5 uses 0)")
        self.channels = channels
        self.emb_channels = emb_channels
        self.dropout = dropout
        self.out_channels = out_channels or channels
        self.use_conv = use_conv
        self.use_checkpoint = use_checkpoint
        self.use_scale_shift_norm = use_scale_shift_norm
        self.updown = False
        self.in_layers = nn.Sequential(
            normalization(channels), nn.SiLU(), conv_nd(dims, channels, self.out_channels, 3, padding=1)
        )
        self.h_upd = self.x_upd = nn.Identity()
        self.emb_layers = nn.Sequential(nn.SiLU(), linear(emb_channels, self.out_channels))
        self.out_layers = nn.Sequential(
            normalization(self.out_channels), nn.SiLU(), nn.Dropout(p=dropout),
            zero_module(conv_nd(dims, self.out_channels, self.out_channels, 3, padding=1)),
        )
        if self.out_channels == channels:
            self.skip_connection = nn.Identity()
        elif use_conv:
            self.skip_connection = conv_nd(dims, channels, self.out_channels, 3, padding=1)
        else:
            self.skip_connection = conv_nd(dims, channels, self.out_channels, 1)
        self._emb_slice = None  # (offset, width) into EmbPack.all_out, assigned by UNetModel

    def hip(self, x, emb):
        """x: [B,H,W,C] fp16 or SkipCat((h, skip)); emb: EmbPack or fp16 [B, emb_ch] (raw emb)."""
        x1, x2 = (x[0], x[1]) if isinstance(x, SkipCat) else (x, None)
        if isinstance(emb, EmbPack) and emb.all_out is not None and self._emb_slice is not None:
            off, width = self._emb_slice
            e = emb.all_out[:, off:off + width]          # [B, Cout] view, row stride = sum(Cout)
        else:
            se = emb.silu_emb if isinstance(emb, EmbPack) else ops.silu(emb.to(F16).contiguous())
            e = self.emb_layers[1].hip(se)
        h = self.in_layers[0].hip(x1, silu=True, x2=x2)
        # both convolutions feed a GroupNorm(32) (this block's second norm; the next block's first norm, a transformer's norm or the output
        # norm): they leave the partial statistics of what they store (Conv2d.hip gn_groups)
        h = self.in_layers[2].hip(h, rowbias=e, gn_groups=32)
        h = self.out_layers[0].hip(h, silu=True)
        if isinstance(self.skip_connection, nn.Identity):
            skip = x1 if x2 is None else torch.cat([x1, x2], dim=-1)
        elif self._skip_fusable(x1, x2):
            return ops.conv3x3(h, self._packed_conv2_skip(), skip=(x1, x2), gn_cpg=self.out_channels // 32)
        else:
            skip = self.skip_connection.hip(x1, x2=x2)
        return self.out_layers[3].hip(h, residual=skip, gn_groups=32)

    # ---- out_layers convolution + channel-changing 1x1 skip_connection as ONE K-concatenated implicit GEMM (ops.pack_conv3x3_skip): the block's
    # `skip_connection(x) + h` (openaimodel.py:256-276) costs no launch, no [B,H,W,Cout] round trip and no residual read of its own
    def _skip_fusable(self, x1, x2) -> bool:
        sc = self.skip_connection
        return (FUSE_SKIP and isinstance(sc, nn.Conv2d) and sc.kernel_size == (1, 1) and self.out_channels % 64 == 0 and x1.shape[-1] % 64 == 0
                and (x2 is None or x2.shape[-1] % 64 == 0))

    def _packed_conv2_skip(self) -> ops.PackedWeight:
        c2, sc = self.out_layers[3], self.skip_connection
        if not hasattr(self, "_cache_c2s"):
            self._cache_c2s = _PackCache()
        return self._cache_c2s.get((c2.weight, c2.bias, sc.weight, sc.bias),
                                   lambda: ops.pack_conv3x3_skip(c2.weight, c2.bias, sc.weight, sc.bias, c2.weight.device))

    def _emb_out(self, emb):
        if isinstance(emb, EmbPack) and emb.all_out is not None and self._emb_slice is not None:
            off, width = self._emb_slice
            return emb.all_out[:, off:off + width]
        se = emb.silu_emb if isinstance(emb, EmbPack) else ops.silu(emb.to(F16).contiguous())
        return self.emb_layers[1].hip(se)

    _lora = None      # {"conv1" | "conv2" | "conv_shortcut": DoRAConvAdapter}: set by _UNetFunction around hip_train (modules/dora.py)

    def hip_train(self, x, emb):
        """hip() keeping what the activation-gradient backward needs: the block input(s), the conv1
        output and the two GroupNorm statistics (GroupNorm outputs are only needed for weight gradients,
        which do not exist here: base weights are frozen, ddpm.py:4131-4132).  With trainable DoRA adapters attached
        (`_lora`) the three convolutions run through modules/dora.py, which keeps its own operands."""
        from ..dora import dora_conv_fwd
        lora = self._lora or {}
        x1, x2 = (x[0], x[1]) if isinstance(x, SkipCat) else (x, None)
        a, st1 = self.in_layers[0].hip_train(x1, silu=True, x2=x2)
        s1 = s2 = ssc = None
        if "conv1" in lora:
            ad = lora["conv1"]
            h1, s1 = dora_conv_fwd(self.in_layers[2], ad, a, rowbias=self._emb_out(emb), mask=ad.draw_mask(a.shape, a.device))
        else:
            h1 = self.in_layers[2].hip(a, rowbias=self._emb_out(emb), gn_groups=32)
        b, st2 = self.out_layers[0].hip_train(h1, silu=True)
        fuse = "conv2" not in lora and "conv_shortcut" not in lora and not isinstance(self.skip_connection, nn.Identity) and self._skip_fusable(x1, x2)
        if fuse:
            skip = None                               # the shortcut runs inside the second convolution (see hip())
        elif isinstance(self.skip_connection, nn.Identity):
            skip = x1 if x2 is None else torch.cat([x1, x2], dim=-1)
        elif "conv_shortcut" in lora:
            ad = lora["conv_shortcut"]
            cin = x1.shape[-1] + (0 if x2 is None else x2.shape[-1])
            skip, ssc = dora_conv_fwd(self.skip_connection, ad, x1, x2=x2, mask=ad.draw_mask(x1.shape[:-1] + (cin,), x1.device))
        else:
            skip = self.skip_connection.hip(x1, x2=x2)
        if fuse:
            out = ops.conv3x3(b, self._packed_conv2_skip(), skip=(x1, x2), gn_cpg=self.out_channels // 32)
        elif "conv2" in lora:
            ad = lora["conv2"]
            out, s2 = dora_conv_fwd(self.out_layers[3], ad, b, residual=skip, mask=ad.draw_mask(b.shape, b.device))
        else:
            out = self.out_layers[3].hip(b, residual=skip, gn_groups=32)
        return out, (x1, x2, st1, h1, st2, (lora, s1, s2, ssc, {}) if lora else None)

    def hip_bwd(self, saved, dy):
        """Reverse of openaimodel.py:256-276 (no gradient flows into the time embedding: it depends on t only).  Adapter
        parameter gradients are left in the dict at the end of `saved`."""
        from ..dora import dora_conv_bwd
        x1, x2, st1, h1, st2, ls = saved
        lora, s1, s2, ssc, grads = ls if ls is not None else ({}, None, None, None, None)
        if s2 is not None:
            db, grads["conv2"] = dora_conv_bwd(self.out_layers[3], lora["conv2"], s2, dy)
        else:
            db = self.out_layers[3].hip_dgrad(dy)
        dh1 = self.out_layers[0].hip_bwd(h1, st2, db, silu=True)
        if s1 is not None:
            da, grads["conv1"] = dora_conv_bwd(self.in_layers[2], lora["conv1"], s1, dh1)
        else:
            da = self.in_layers[2].hip_dgrad(dh1)
        if isinstance(self.skip_connection, nn.Identity):
            dskip = dy
        elif ssc is not None:
            dskip, grads["conv_shortcut"] = dora_conv_bwd(self.skip_connection, lora["conv_shortcut"], ssc, dy)
        else:
            dskip = self.skip_connection.hip_dgrad(dy)
        return self.in_layers[0].hip_bwd(x1, st1, da, silu=True, x2=x2, add=dskip)

    def forward(self, x, emb):
        return checkpoint(self._forward, (x, emb), self.parameters(), self.use_checkpoint)

    def _forward(self, x, emb):
        return from_nhwc_f16(self.hip(to_nhwc_f16(x), emb), x.dtype)


def _kv_all_pack(net, layers):
    """The stacked [all to_k | all to_v] weights of ``net``'s cross-attention ``layers``, packed once per weight version (a module-level function:
    ControlNet borrows ``UNetModel._project_context_all``, which calls it)."""
    ws = [m.to_k.weight for m in layers] + [m.to_v.weight for m in layers]
    if not hasattr(net, "_kv_all_cache"):
        net._kv_all_cache = _PackCache()
    return net._kv_all_cache.get(ws, lambda: ops.pack_matrix(torch.cat([w.detach() for w in ws], 0), None, ws[0].device))


def check_freeu_values(who, b1, b2, s1, s2, version):
    """ValueError (naming ``who`` and the argument) unless b1, b2, s1, s2 are finite numbers >= 0 and version is 1 or 2 -> the checked dict."""
    out = {}
    for name, v in (("b1", b1), ("b2", b2), ("s1", s1), ("s2", s2)):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"{who}: {name} must be a number, got {type(v).__name__}")
        v = float(v)
        if v != v or v in (float("inf"), float("-inf")) or v < 0:
            raise ValueError(f"{who}: {name} must be finite and >= 0, got {v}")
        out[name] = v
    if isinstance(version, bool) or version not in (1, 2):
        raise ValueError(f"{who}: version must be 1 or 2, got {version!r}")
    out["version"] = int(version)
    return out


def freeu_plan(model_channels, h_channels, cfg):
    """FreeU's per-output-block plan: for each output block, given the channels of h in front of its skip concatenation, (b1, s1) where h has
    4 x model_channels, (b2, s2) where it has 2 x model_channels, None elsewhere (the authors' patch of the ldm UNetModel keys the stages by
    channel count).  ``cfg``: set_freeu's state or None (every block None).  Pure: no device, no module."""
    if cfg is None:
        return [None] * len(h_channels)
    stage = {4 * model_channels: (cfg["b1"], cfg["s1"]), 2 * model_channels: (cfg["b2"], cfg["s2"])}
    return [stage.get(c) for c in h_channels]


class UNetModel(nn.Module):
    """The SD-1.5 U-Net with the reference's constructor signature (openaimodel.py:444-469).
    Only the options SD-1.5 uses are implemented; the others raise at construction."""

    def __init__(self, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions, dropout=0,
                 channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2, num_classes=None, use_checkpoint=False,
                 use_fp16=False, num_heads=-1, num_head_channels=-1, num_heads_upsample=-1, use_scale_shift_norm=False,
                 resblock_updown=False, use_new_attention_order=False, use_spatial_transformer=False, transformer_depth=1,
                 context_dim=None, n_embed=None, legacy=True):
        super().__init__()
        if not use_spatial_transformer or context_dim is None:
            raise NotImplementedError("only the use_spatial_transformer=True / context_dim path (SD-1.x) is implemented")
        if num_classes is not None or n_embed is not None or resblock_updown or use_scale_shift_norm or dims != 2:
            raise NotImplementedError("class-conditional / codebook / resblock_updown / scale-shift variants are off the hot path")
        if isinstance(context_dim, (list, tuple)) or type(context_dim).__name__ == "ListConfig":
            context_dim = list(context_dim)[0]
        if num_heads_upsample == -1:
            num_heads_upsample = num_heads
        if num_heads == -1 and num_head_channels == -1:
            raise ValueError("Either num_heads or num_head_channels has to be set")

        self.in_channels = in_channels
        self.model_channels = model_channels
        self.out_channels = out_channels
        self.num_res_blocks = num_res_blocks
        self.attention_resolutions = attention_resolutions
        self.dropout = dropout
        self.channel_mult = channel_mult
        self.conv_resample = conv_resample
        self.num_classes = num_classes
        self.use_checkpoint = use_checkpoint
        self.dtype = torch.float16 if use_fp16 else torch.float32
        self.num_heads = num_heads
        self.num_head_channels = num_head_channels
        self.num_heads_upsample = num_heads_upsample
        self.predict_codebook_ids = False
        self.debug_attn = False
        self.backup_vars = {"save_cross_attn_vars": False}

        def heads_of(ch, nh):
            if num_head_channels == -1:
                return nh, ch // nh
            return ch // num_head_channels, num_head_channels

        def transformer(ch, nh):
            n, d = heads_of(ch, nh)
            return SpatialTransformer(ch, n, d, depth=transformer_depth, context_dim=context_dim)

        time_embed_dim = model_channels * 4
        self.time_embed = nn.Sequential(linear(model_channels, time_embed_dim), nn.SiLU(), linear(time_embed_dim, time_embed_dim))

        conv_in = conv_nd(dims, in_channels, model_channels, 3, padding=1)
        conv_in.cin_pad = ops.round_up(in_channels, 8)
        self.input_blocks = nn.ModuleList([TimestepEmbedSequential(conv_in)])
        input_block_chans = [model_channels]
        ch = model_channels
        ds = 1
        for level, mult in enumerate(channel_mult):
            for _ in range(num_res_blocks):
                layers = [ResBlock(ch, time_embed_dim, dropout, out_channels=mult * model_channels, dims=dims,
                                   use_checkpoint=use_checkpoint)]
                ch = mult * model_channels
                if ds in attention_resolutions:
                    layers.append(transformer(ch, num_heads))
                self.input_blocks.append(TimestepEmbedSequential(*layers))
                input_block_chans.append(ch)
            if level != len(channel_mult) - 1:
                self.input_blocks.append(TimestepEmbedSequential(Downsample(ch, conv_resample, dims=dims, out_channels=ch)))
                input_block_chans.append(ch)
                ds *= 2

        self.middle_block = TimestepEmbedSequential(
            ResBlock(ch, time_embed_dim, dropout, dims=dims, use_checkpoint=use_checkpoint),
            transformer(ch, num_heads),
            ResBlock(ch, time_embed_dim, dropout, dims=dims, use_checkpoint=use_checkpoint),
        )

        self.output_blocks = nn.ModuleList([])
        self._out_h_channels = []                # channels of h in front of each output block's skip concatenation (freeu_plan keys FreeU's stages by them)
        for level, mult in list(enumerate(channel_mult))[::-1]:
            for i in range(num_res_blocks + 1):
                ich = input_block_chans.pop()
                self._out_h_channels.append(ch)
                layers = [ResBlock(ch + ich, time_embed_dim, dropout, out_channels=model_channels * mult, dims=dims,
                                   use_checkpoint=use_checkpoint)]
                ch = model_channels * mult
                if ds in attention_resolutions:
                    layers.append(transformer(ch, num_heads_upsample))
                if level and i == num_res_blocks:
                    layers.append(Upsample(ch, conv_resample, dims=dims, out_channels=ch))
                    ds //= 2
                self.output_blocks.append(TimestepEmbedSequential(*layers))

        self.out = nn.Sequential(
            normalization(ch), nn.SiLU(), zero_module(conv_nd(dims, model_channels, out_channels, 3, padding=1))
        )

        self._assign_emb_slices()
        self.__dict__["_control"] = None         # set_control's state ({"net", "hint", "scale", "expanded", "active"}) while it holds a ControlNet; not a submodule either
        self.__dict__["_ip"] = None              # set_ip_adapter's state ({"adapter", "rows", "T", "kv", "scale", "active"}) while it holds an IP-Adapter; not a submodule
        self.__dict__["_regions"] = None         # set_regions' state ({"rows", "R", "L", "k", "vt", "w"}) while regional prompts are set; not a submodule
        self.__dict__["_freeu"] = None           # set_freeu's state ({"b1", "b2", "s1", "s2", "version"}) while FreeU is set; plain numbers, not in the state dict
        self.__dict__["_motion"] = None          # (MotionModule, num_frames) while set_motion holds one; not a submodule: the state dict stays SD-1.5's

    # ------------------------------------------------------------------ reference flag plumbing
    ALL_CA_LAYER_INDICES = [1, 2, 4, 5, 7, 8, 12, 16, 17, 18, 19, 20, 21, 22, 23, 24]  # openaimodel.py:721

    def _layer_blocks(self):
        return list(self.input_blocks) + [self.middle_block] + list(self.output_blocks)

    def set_cross_attn_flags(self, ca_flag_dict=None, ca_layer_indices=None, trans_flag_dict=None, trans_layer_indices=None):
        """Set attributes on attn2 (ca_flag_dict) / the transformer block (trans_flag_dict) of the
        selected cross-attention layers; returns the previous values (openaimodel.py:716-817).
        The ':layerwise' / ':layerwise-dict' value forms of the reference are accepted."""
        if ca_flag_dict is None and trans_flag_dict is None:
            return None, None
        l2ca = {li: i for i, li in enumerate(self.ALL_CA_LAYER_INDICES)}
        blocks = self._layer_blocks()

        def apply(flag_dict, indices, target):
            if flag_dict is None or len(indices) == 0:
                return None
            old = {}
            for k, v in flag_dict.items():
                old[k] = self.backup_vars.get(k)
                self.backup_vars[k] = v
                key, lw_arr, lw_dict = k, False, False
                if key.endswith(":layerwise"):
                    key, lw_arr = key[: -len(":layerwise")], v is not None
                if key.endswith(":layerwise-dict"):
                    key, lw_dict = key[: -len(":layerwise-dict")], v is not None
                for li in indices:
                    if li >= len(blocks) or li not in l2ca:
                        continue
                    blk = blocks[li][1].transformer_blocks[0]
                    if lw_arr:
                        v2 = v[l2ca[li]]
                    elif lw_dict:
                        v2 = v.get(li, None) if hasattr(v, "get") else v
                    else:
                        v2 = v
                    (blk.attn2 if target == "ca" else blk).__dict__[key] = v2
            return old

        ca_idx = self.ALL_CA_LAYER_INDICES if ca_layer_indices is None else ca_layer_indices
        tr_idx = self.ALL_CA_LAYER_INDICES if trans_layer_indices is None else trans_layer_indices
        return apply(ca_flag_dict, ca_idx, "ca"), apply(trans_flag_dict, tr_idx, "trans")

    # ------------------------------------------------------------------ packing
    def _assign_emb_slices(self):
        """The batched emb_layers projection: slices assigned in module order."""
        self._resblocks = [m for m in self.modules() if isinstance(m, ResBlock)]
        off = 0
        for rb in self._resblocks:
            rb._emb_slice = (off, rb.out_channels)
            off += ops.round_up(rb.out_channels, 8)
        self._emb_total = off
        self._emb_cache = _PackCache()

    def _packed_emb_all(self):
        params = []
        for rb in self._resblocks:
            params += [rb.emb_layers[1].weight, rb.emb_layers[1].bias]

        def build():
            dev = params[0].device
            K = self._resblocks[0].emb_channels
            w = torch.zeros((self._emb_total, K), dtype=torch.float32, device=dev)
            b = torch.zeros((self._emb_total,), dtype=torch.float32, device=dev)
            for rb in self._resblocks:
                off, width = rb._emb_slice
                w[off:off + width] = rb.emb_layers[1].weight.detach().float()
                b[off:off + width] = rb.emb_layers[1].bias.detach().float()
            return ops.pack_matrix(w, b, dev)

        return self._emb_cache.get(params, build)

    def prepare(self):
        """Pack every weight for the current device now (otherwise done lazily on first use)."""
        for m in self.modules():
            if hasattr(m, "packed"):
                m.packed()
            if hasattr(m, "_packed_qkv") and m.to_k.in_features == m.to_q.in_features:
                m._packed_qkv()
            if hasattr(m, "_packed_kv") and m.to_k.in_features != m.to_q.in_features:
                m._packed_kv()
        self._packed_emb_all()
        return self

    # ------------------------------------------------------------------ video (ldm/modules/motion_module.py)
    def set_motion(self, motion, num_frames=0):
        """Run ``motion`` (a MotionModule) inside ``hip`` on batches of whole ``num_frames``-frame videos (row ``v * F + f``); ``None`` restores the
        image walk exactly.  Refuses (ValueError) a module whose widths do not match this U-Net or a frame count outside 1 .. its max_len."""
        if motion is None:
            self.__dict__["_motion"] = None
            return
        self._refuse_regions("set_motion (video)")
        F = int(num_frames)
        if not 1 <= F <= motion.max_len:
            raise ValueError(f"set_motion: num_frames must be in 1 .. {motion.max_len} (the module's position table), got {num_frames}")
        if len(self.channel_mult) != 4 or self.num_res_blocks != 2:
            raise ValueError("set_motion: motion modules are placed on the SD-1.5 topology (4 levels of 2 ResBlocks)")
        for (where, n), tt in motion.placed():
            block = self.middle_block if where == "middle" else (self.input_blocks if where == "input" else self.output_blocks)[n]
            ch = block[0].out_channels
            if tt.channels != ch:
                raise ValueError(f"set_motion: the module's transformer at {where} block {n} has {tt.channels} channels, the U-Net {ch}")
        self.__dict__["_motion"] = (motion, F)

    def _refuse_motion(self, what):
        if self._motion is not None:
            raise NotImplementedError(f"{what} is not built for video: unset the motion module (set_motion(None)) first")

    # ------------------------------------------------------------------ ControlNet (ldm/modules/diffusionmodules/controlnet.py)
    def set_control(self, controlnet, hint_features=None, scale=1.0):
        """Run ``controlnet`` (a ControlNet) inside ``hip``: after this U-Net's input blocks the ControlNet walks the same latents and adds
        ``scale`` x its thirteen zero-convolution outputs to the twelve skips and to the middle block's output, each join in the epilogue of
        the zero convolution's GEMM.  ``hint_features``: ``controlnet.hint_features(images)``, fp16 [B0, h, w, model_channels]; row b of a
        batch takes hint b % B0.  ``None`` restores the plain walk exactly.  Refuses (ValueError) a ControlNet whose widths or topology do
        not match this U-Net, and, when run, a batch that is not a multiple of B0 or latents of another size than the hints."""
        if controlnet is None:
            self.__dict__["_control"] = None
            return
        for name in ("in_channels", "model_channels", "num_res_blocks", "num_heads", "num_head_channels"):
            if getattr(controlnet, name) != getattr(self, name):
                raise ValueError(f"set_control: the ControlNet's {name} is {getattr(controlnet, name)}, the U-Net's {getattr(self, name)}")
        for name in ("channel_mult", "attention_resolutions"):
            if list(getattr(controlnet, name)) != list(getattr(self, name)):
                raise ValueError(f"set_control: the ControlNet's {name} is {list(getattr(controlnet, name))}, the U-Net's {list(getattr(self, name))}")
        if len(controlnet.input_blocks) != len(self.input_blocks) or len(controlnet.zero_convs) != len(self.input_blocks):
            raise ValueError(f"set_control: the ControlNet has {len(controlnet.input_blocks)} input blocks, the U-Net {len(self.input_blocks)}")
        for n, (a, b) in enumerate(zip(controlnet.input_blocks, self.input_blocks)):
            if [type(m) for m in a] != [type(m) for m in b]:
                raise ValueError(f"set_control: input block {n} of the ControlNet does not have the U-Net's layers")
        cn_ctx, own_ctx = controlnet._cross_attn_layers(), self._cross_attn_layers()
        if cn_ctx and own_ctx and cn_ctx[0].to_k.in_features != own_ctx[0].to_k.in_features:
            raise ValueError(f"set_control: the ControlNet's context_dim is {cn_ctx[0].to_k.in_features}, the U-Net's {own_ctx[0].to_k.in_features}")
        h = hint_features
        if not torch.is_tensor(h) or h.dtype != F16 or h.dim() != 4 or h.shape[0] < 1 or h.shape[3] != self.model_channels:
            raise ValueError(f"set_control: hint_features must be fp16 [B0, h, w, {self.model_channels}] (ControlNet.hint_features), got "
                             f"{(h.dtype, tuple(h.shape)) if torch.is_tensor(h) else type(h).__name__}")
        scale = float(scale)
        if scale != scale or scale in (float("inf"), float("-inf")):
            raise ValueError(f"set_control: scale must be finite, got {scale}")
        self.__dict__["_control"] = {"net": controlnet, "hint": h.contiguous(), "scale": scale, "expanded": {}, "active": True}

    def set_control_active(self, active):
        """Switch the ControlNet that is set off or on between two steps (a guidance window) without dropping its expanded hints; while it
        is off, ``hip`` is the plain walk.  Everything ``_refuse_control`` refuses stays refused until ``set_control(None)``."""
        if self._control is None:
            raise ValueError("set_control_active: no ControlNet is set")
        self._control["active"] = bool(active)

    def _refuse_control(self, what):
        if self._control is not None:
            raise NotImplementedError(f"{what} is not built with a ControlNet: unset it (set_control(None)) first")

    # ------------------------------------------------------------------ IP-Adapter (adaface/ip_adapter.py)
    def check_ip_adapter(self, adapter):
        """ValueError unless ``adapter``'s to_k_ip / to_v_ip fit this U-Net's cross-attention layers one to one -> those layers."""
        layers = self._cross_attn_layers()
        if len(adapter.to_k_ip) != len(layers) or len(adapter.to_v_ip) != len(layers):
            raise ValueError(f"set_ip_adapter: the adapter has {len(adapter.to_k_ip)} to_k_ip / {len(adapter.to_v_ip)} to_v_ip layers, the U-Net "
                             f"{len(layers)} cross-attention layers")
        for j, (m, wk, wv) in enumerate(zip(layers, adapter.to_k_ip, adapter.to_v_ip)):
            for name, w in (("to_k_ip", wk), ("to_v_ip", wv)):
                if (w.out_features, w.in_features) != (m.inner_dim, m.to_k.in_features):
                    raise ValueError(f"set_ip_adapter: {name} of layer {j} maps {w.in_features} -> {w.out_features}, the U-Net's layer "
                                     f"{m.to_k.in_features} -> {m.inner_dim}")
        return layers

    def set_ip_adapter(self, adapter, cond_tokens=None, uncond_tokens=None, scale=1.0):
        """Run ``hip`` with ``adapter``'s (an IPAdapter) decoupled cross-attention: every one of this U-Net's cross-attention layers adds
        ``scale`` x the softmax over the image tokens to its text attention (af_ip_attention_add, one launch per layer).  ``cond_tokens`` /
        ``uncond_tokens``: fp16 [rows, T, context_dim] from ``adapter.image_proj``.  Both sets are projected HERE, once, for all layers by ONE
        GEMM over the adapter's stacked [all to_k_ip | all to_v_ip] weights; a step only adds the launches.  A batch of ``rows`` runs the cond
        tokens, a batch of 2 x rows cond then uncond (the samplers' order, sampling.py::_eps); any other batch is a ValueError.  A ControlNet
        set beside it sees the text only.  ``None`` restores the plain walk exactly, the one-launch routes included."""
        if adapter is None:
            self.__dict__["_ip"] = None
            return
        layers = self.check_ip_adapter(adapter)
        cc = layers[0].to_k.in_features
        for name, t in (("cond_tokens", cond_tokens), ("uncond_tokens", uncond_tokens)):
            if not torch.is_tensor(t) or t.dtype != F16 or t.dim() != 3 or t.shape[0] < 1 or t.shape[2] != cc or not 1 <= t.shape[1] <= ops.IP_ATTN_MAX_TOKENS:
                raise ValueError(f"set_ip_adapter: {name} must be fp16 [rows, 1 <= T <= {ops.IP_ATTN_MAX_TOKENS}, {cc}], got "
                                 f"{(t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}")
        if cond_tokens.shape != uncond_tokens.shape:
            raise ValueError(f"set_ip_adapter: cond_tokens are {tuple(cond_tokens.shape)}, uncond_tokens {tuple(uncond_tokens.shape)}")
        scale = float(scale)
        if scale != scale or scale in (float("inf"), float("-inf")):
            raise ValueError(f"set_ip_adapter: scale must be finite, got {scale}")
        rows, T, _ = cond_tokens.shape
        pack = adapter.packed_kv()                                                # [all to_k_ip | all to_v_ip], packed once per weight version
        kv = ops.gemm(torch.cat([cond_tokens, uncond_tokens], 0).reshape(2 * rows * T, cc).contiguous(), pack)
        self.__dict__["_ip"] = {"adapter": adapter, "rows": rows, "T": T, "kv": kv.reshape(2 * rows, T, kv.shape[1]), "scale": scale, "active": True}

    def set_ip_adapter_active(self, active):
        """Switch the IP-Adapter that is set off or on between two steps (a guidance window) without dropping its projected tokens; while it
        is off, ``hip`` is the plain walk.  Everything ``_refuse_ip`` refuses stays refused until ``set_ip_adapter(None)``."""
        if self._ip is None:
            raise ValueError("set_ip_adapter_active: no IP-Adapter is set")
        self._ip["active"] = bool(active)

    def _refuse_ip(self, what):
        if self._ip is not None:
            raise NotImplementedError(f"{what} is not built with an IP-Adapter: unset it (set_ip_adapter(None)) first")

    def _place_ip(self, B):
        """Hand every cross-attention layer its slice of the projected image tokens for a batch of B rows -> the layers to clear afterwards."""
        ip = self._ip
        if ip is None or not ip["active"]:
            return []
        if B not in (ip["rows"], 2 * ip["rows"]):
            raise ValueError(f"the batch ({B}) is neither the image tokens' rows ({ip['rows']}: cond) nor twice that (cond, then uncond)")
        layers = self._cross_attn_layers()
        kv = ip["kv"][:B]
        sc = kv.shape[2] // 2
        off = 0
        for m in layers:
            c = m.inner_dim
            m._ip_pre = (kv[:, :, off:off + c], kv[:, :, sc + off:sc + off + c], ip["scale"])
            off += c
        return layers

    # ------------------------------------------------------------------ regional prompts (several subjects)
    def set_regions(self, contexts, uncond_context=None, weights=None):
        """Run ``hip`` with regional prompts: every cross-attention layer attends to R context sets per batch row -- set 0 the base prompt, sets
        1 .. R-1 the regions -- and blends the results per token under the region weights (af_region_attention, one launch per layer).
        ``contexts``: fp16 [rows, R, L, context_dim]; ``uncond_context``: fp16 [rows, L, context_dim]; ``weights``: the levels' fp32 device
        tensors [R, N_l] (``ops.region_weights``), one per token count a cross-attention layer of this U-Net will see.  All layers' K | V^T of all
        sets are projected HERE, once, by ONE GEMM over the stacked [all to_k | all to_v] weights with the sets as batch items; a step adds no
        projection GEMM.  A batch of ``rows`` runs cond, a batch of 2 x rows cond then uncond (the samplers' order); anything else is a ValueError.
        The uncond rows run their context under w = (1, 0, ..., 0): their sets 1 .. R-1 are never read and are not projected.  ``hip`` is still
        given the base context (cond, uncond), which a ControlNet set beside this U-Net reads.  ``None`` restores the plain walk exactly, the
        one-launch routes included."""
        if contexts is None:
            self.__dict__["_regions"] = None
            return
        self._refuse_motion("set_regions")
        layers = self._cross_attn_layers()
        if not layers:
            raise ValueError("set_regions: this U-Net has no cross-attention layer")
        cc = layers[0].to_k.in_features
        c = contexts
        if (not torch.is_tensor(c) or c.dtype != F16 or c.dim() != 4 or c.shape[0] < 1 or c.shape[3] != cc or not 1 <= c.shape[1] <= ops.REGION_MAX
                or not 1 <= c.shape[2] <= ops.REGION_MAX_TOKENS):
            raise ValueError(f"set_regions: contexts must be fp16 [rows, 1 <= R <= {ops.REGION_MAX}, 1 <= L <= {ops.REGION_MAX_TOKENS}, {cc}], got "
                             f"{(c.dtype, tuple(c.shape)) if torch.is_tensor(c) else type(c).__name__}")
        rows, R, L, _ = c.shape
        u = uncond_context
        if not torch.is_tensor(u) or u.dtype != F16 or tuple(u.shape) != (rows, L, cc):
            raise ValueError(f"set_regions: uncond_context must be fp16 [{rows}, {L}, {cc}], got "
                             f"{(u.dtype, tuple(u.shape)) if torch.is_tensor(u) else type(u).__name__}")
        if not isinstance(weights, (list, tuple)) or not weights:
            raise ValueError("set_regions: weights must be the levels' fp32 tensors [R, N_l] (ops.region_weights)")
        for t in weights:
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != R or t.shape[1] < 1:
                raise ValueError(f"set_regions: every level's weights must be fp32 [{R}, N_l], got "
                                 f"{(t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}")
        if len({t.shape[1] for t in weights}) != len(weights):
            raise ValueError(f"set_regions: two levels of weights have the same token count ({[t.shape[1] for t in weights]})")
        dev = c.device
        pack = _kv_all_pack(self, layers)
        sc = pack.N // 2
        # the projected items: rows x R cond sets, then the rows' uncond contexts; placed as batch item b R + r of a [2 rows R] stack whose
        # uncond sets 1 .. R-1 stay zero (weight 0: never read)
        src = torch.cat([c.reshape(rows * R, L, cc), u.to(dev)], 0).reshape((rows * R + rows) * L, cc).contiguous()
        k_p, vt_p = ops.gemm(src, pack, rows_per_batch=L, split_col=sc)
        k = torch.zeros((2 * rows * R * L, sc), dtype=F16, device=dev)
        vt = torch.zeros((2 * rows * R,) + tuple(vt_p.shape[1:]), dtype=F16, device=dev)
        k[:rows * R * L] = k_p[:rows * R * L]
        vt[:rows * R] = vt_p[:rows * R]
        k[rows * R * L:].reshape(rows, R, L, sc)[:, 0] = k_p[rows * R * L:].reshape(rows, L, sc)
        vt[rows * R:].reshape((rows, R) + tuple(vt_p.shape[1:]))[:, 0] = vt_p[rows * R:]
        w = {}
        for t in weights:
            full = torch.zeros((2 * rows, R, t.shape[1]), dtype=torch.float32, device=dev)
            full[:rows] = t.to(dev)[None]
            full[rows:, 0] = 1.0
            w[t.shape[1]] = full.reshape(2 * rows * R, t.shape[1])
        self.__dict__["_regions"] = {"rows": rows, "R": R, "L": L, "k": k, "vt": vt, "w": w}

    def _refuse_regions(self, what):
        if self._regions is not None:
            raise NotImplementedError(f"{what} is not built with regional prompts: unset them (set_regions(None)) first")

    # ------------------------------------------------------------------ FreeU (csrc/af_freeu.hip)
    def set_freeu(self, b1, b2=None, s1=None, s2=None, version=2):
        """Run ``hip`` with FreeU (Si et al.): in front of every output block whose h has 4 x model_channels (b1, s1) or 2 x model_channels
        (b2, s2) channels, the first half of h's channels is boosted and the skip loses part of its lowest spatial frequencies (``freeu_plan``,
        ``ops.freeu``: two launches per block, in place).  The joined skip is what is filtered when a ControlNet is set.  ``set_freeu(None)``
        restores the plain walk exactly, and so do four values of 1 (no launch).  Not built for training and the trunk cache (refused by name)."""
        if b1 is None:
            self.__dict__["_freeu"] = None
            return
        self.__dict__["_freeu"] = check_freeu_values("set_freeu", b1, b2, s1, s2, version)

    def freeu_plan(self):
        """[(b, s) | None] per output block for the FreeU state that is set (``freeu_plan`` of this module)."""
        return freeu_plan(self.model_channels, self._out_h_channels, self._freeu)

    def _refuse_freeu(self, what):
        if self._freeu is not None:
            raise NotImplementedError(f"{what} is not built with FreeU: unset it (set_freeu(None)) first")

    def _place_regions(self, B, L=None):
        """Hand every cross-attention layer (k, vt, ldk, vt_batch_stride, {N: w_level}, R) -- its slices of the stacked projection of all context
        sets -- for a batch of B rows -> the layers to clear afterwards."""
        rg = self._regions
        if rg is None:
            return []
        if B not in (rg["rows"], 2 * rg["rows"]):
            raise ValueError(f"the batch ({B}) is neither the regions' rows ({rg['rows']}: cond) nor twice that (cond, then uncond)")
        if L is not None and L != rg["L"]:
            raise ValueError(f"the context has {L} tokens, the regions' contexts {rg['L']}")
        layers = self._cross_attn_layers()
        R = rg["R"]
        k, vt = rg["k"][:B * R * rg["L"]], rg["vt"][:B * R]
        w = {n: t[:B * R] for n, t in rg["w"].items()}
        off = 0
        for m in layers:
            c = m.inner_dim
            m._region_pre = (k[:, off:off + c], vt[:, off:off + c, :], k.stride(0), vt.stride(0), w, R)
            off += c
        return layers

    def _control_hint(self, B, hw):
        """The hint features for a batch of B rows (row b: hint b % B0), expanded once per batch size and kept."""
        ctrl = self._control
        hint = ctrl["hint"]
        B0 = hint.shape[0]
        if B % B0:
            raise ValueError(f"the batch ({B}) is not a multiple of the hint batch ({B0})")
        if tuple(hint.shape[1:3]) != tuple(hw):
            raise ValueError(f"the hints are for {hint.shape[1]} x {hint.shape[2]} latents, the batch holds {hw[0]} x {hw[1]}")
        if B not in ctrl["expanded"]:
            ctrl["expanded"][B] = hint if B == B0 else hint.repeat(B // B0, 1, 1, 1)
        return ctrl["expanded"][B]

    def _hip_block_motion(self, module, where, n, h, emb, context, img_mask):
        """``module.hip`` with the temporal transformer placed at (where, n), if any: behind an input block, between the middle block's
        SpatialTransformer and its second ResBlock, in front of an output block's Upsample."""
        motion, F = self._motion
        tt = motion.at(where, n)
        if tt is None:
            return module.hip(h, emb, context, img_mask)
        if h[0].shape[0] % F if isinstance(h, SkipCat) else h.shape[0] % F:
            raise ValueError(f"the batch ({(h[0] if isinstance(h, SkipCat) else h).shape[0]}) is not a multiple of num_frames ({F})")
        done = False
        for k, layer in enumerate(module):
            if not done and (isinstance(layer, Upsample) or (where == "middle" and k == 2)):
                h, done = tt.hip(h, F), True
            if isinstance(layer, TimestepBlock):
                h = layer.hip(h, emb)
            elif isinstance(layer, SpatialTransformer):
                h = layer.hip(h, context, img_mask)
            else:
                h = layer.hip(h)
        return h if done else tt.hip(h, F)

    # ------------------------------------------------------------------ forward
    def hip(self, x_nhwc, timesteps, context, img_mask=None, capture_layers=()):
        """x_nhwc [B,H,W,8] fp16 (4 latent channels + zero pad), timesteps int64 [B],
        context [B,L,ctx] fp16 -> (eps [B,H,W,out_channels] fp16, captured activations)."""
        if capture_layers:
            self._refuse_ip("capturing cross-attention activations")
            self._refuse_regions("capturing cross-attention activations")
        emb = self._embed(timesteps)   # SiLU(emb) (its only consumers are the emb_layers) + all 22 projections
        kv_layers = self._project_context_all(context)
        ip_layers, rg_layers = [], []
        try:
            ip_layers = self._place_ip(x_nhwc.shape[0])
            rg_layers = self._place_regions(x_nhwc.shape[0], None if context is None else context.shape[1])
            return self._hip_blocks(x_nhwc, emb, context, img_mask, capture_layers, timesteps)
        finally:
            for m in kv_layers:
                m._kv_pre = None
            for m in ip_layers:
                m._ip_pre = None
            for m in rg_layers:
                m._region_pre = None

    def _cross_attn_layers(self):
        out = []
        for blocks in (self.input_blocks, [self.middle_block], self.output_blocks):
            for module in blocks:
                for layer in module:
                    if isinstance(layer, SpatialTransformer):
                        out += [tb.attn2 for tb in layer.transformer_blocks]
        return out

    def _project_context_all(self, context):
        """The K and V^T projections of the context for ALL cross-attention layers in ONE GEMM (they depend on the context only):
        weights stacked [all to_k | all to_v] -> k_all [B*L, sum_C] and, through the transposing epilogue, vt_all [B, sum_C, ld];
        every layer then reads its column / row slice in place (row stride sum_C, vt batch stride sum_C * ld).  16 launches of
        ~10 us with M = 616 rows become one."""
        layers = self._cross_attn_layers()
        if not layers or context is None:
            return []
        pack = _kv_all_pack(self, layers)
        B, L, cc = context.shape
        sc = pack.N // 2
        k_all, vt_all = ops.gemm(context.reshape(B * L, cc), pack, rows_per_batch=L, split_col=sc)
        off = 0
        for m in layers:
            c = m.inner_dim
            m._kv_pre = (k_all[:, off:off + c], vt_all[:, off:off + c, :], sc)
            off += c
        return layers

    def _hip_blocks(self, x_nhwc, emb, context, img_mask, capture_layers, timesteps=None):
        acts = {}
        hs = []
        h = x_nhwc
        layer_idx = 0

        def collect(module, h):
            attn2 = module[1].transformer_blocks[0].attn2
            a = attn2.cached_activations
            a["outfeat"] = from_nhwc_f16(h, torch.float32)
            acts[layer_idx] = a
            attn2.cached_activations = None

        if self._motion is None:
            def run(module, where, n, h):
                return module.hip(h, emb, context, img_mask)
        else:
            if capture_layers:
                raise NotImplementedError("capturing cross-attention activations is not built for video")

            def run(module, where, n, h):
                return self._hip_block_motion(module, where, n, h, emb, context, img_mask)

        for n, module in enumerate(self.input_blocks):
            h = run(module, "input", n, h)
            hs.append(h)
            if layer_idx in capture_layers:
                collect(module, h)
            layer_idx += 1
        ctrl = self._control if self._control is not None and self._control["active"] else None
        if ctrl is not None:
            # the ControlNet walks the same latents (per frame, without temporal layers, when a motion module is set too) and hands back the
            # joined skips as fresh tensors; the middle residual is joined behind this U-Net's middle block
            hint = self._control_hint(x_nhwc.shape[0], x_nhwc.shape[1:3])
            hs, mid = ctrl["net"].hip_walk(x_nhwc, timesteps, context, hint, hs, ctrl["scale"], img_mask)
        h = run(self.middle_block, "middle", 1, h)
        if ctrl is not None:
            h = ctrl["net"].join_middle(mid, h, ctrl["scale"])
        if layer_idx in capture_layers:
            collect(self.middle_block, h)
        layer_idx += 1
        fu = self._freeu
        plan = self.freeu_plan() if fu is not None else [None] * len(self.output_blocks)
        for n, module in enumerate(self.output_blocks):
            skip = hs.pop()
            if plan[n] is not None:
                # FreeU, in place on both: h is the previous block's output and the skip an input block's (or the ControlNet's joined one), each
                # read by nobody else from here on; ops.freeu drops the producers' GroupNorm statistics of what it rewrites
                h, skip = ops.freeu(h, skip, plan[n][0], plan[n][1], fu["version"], out_h=h, out_skip=skip)
            h = run(module, "output", n, SkipCat((h, skip)))
            if layer_idx in capture_layers:
                collect(module, h)
            layer_idx += 1
        h = self.out[0].hip(h, silu=True)
        return self.out[2].hip(h), acts

    def hip_tail(self, trunk, timesteps, context, capture_layers, n_tail=3):
        """The inference walk of the last ``n_tail`` decoder blocks + the output head on trunk = (h, skips) as ``hip_trunk`` returns them
        (a step's shared gradient-free trunk, LatentDiffusion.guided_denoise): -> (eps NHWC, captured activations) exactly as ``_hip_blocks``
        leaves them for those layers."""
        self._refuse_motion("the trunk cache (hip_tail)")
        self._refuse_control("the trunk cache (hip_tail)")
        self._refuse_ip("the trunk cache (hip_tail)")
        self._refuse_regions("the trunk cache (hip_tail)")
        self._refuse_freeu("the trunk cache (hip_tail)")
        h, skips = trunk
        emb = self._embed(timesteps)
        kv_layers = self._project_context_all(context)
        acts = {}
        try:
            n_out = len(self.output_blocks)
            layer_idx = len(self.input_blocks) + 1 + n_out - n_tail
            for k, module in enumerate(list(self.output_blocks)[n_out - n_tail:]):
                h = module.hip(SkipCat((h, skips[k])), emb, context, None)
                if layer_idx in capture_layers:
                    attn2 = module[1].transformer_blocks[0].attn2
                    a = attn2.cached_activations
                    a["outfeat"] = from_nhwc_f16(h, torch.float32)
                    acts[layer_idx] = a
                    attn2.cached_activations = None
                layer_idx += 1
            h = self.out[0].hip(h, silu=True)
            return self.out[2].hip(h), acts
        finally:
            for m in kv_layers:
                m._kv_pre = None

    def _embed(self, timesteps):
        t_emb = timestep_embedding(timesteps, self.model_channels)
        e0 = ops.gemm(t_emb, self.time_embed[0].packed(), act=AF_ACT_SILU)
        semb = ops.gemm(e0, self.time_embed[2].packed(), act=AF_ACT_SILU)
        return EmbPack(semb, ops.gemm(semb, self._packed_emb_all()))

    def hip_train(self, x_nhwc, timesteps, context, img_mask=None):
        """Forward that keeps the activations the backward needs.  -> (eps [B,H,W,out_channels], saved)."""
        self._refuse_motion("hip_train")
        self._refuse_control("hip_train")
        self._refuse_ip("hip_train")
        self._refuse_regions("hip_train")
        self._refuse_freeu("hip_train")
        emb = self._embed(timesteps)
        saved_in, saved_out, hs = [], [], []
        h = x_nhwc
        for module in self.input_blocks:
            h, s = module.hip_train(h, emb, context, img_mask)
            saved_in.append(s)
            hs.append(h)
        h, saved_mid = self.middle_block.hip_train(h, emb, context, img_mask)
        for module in self.output_blocks:
            h, s = module.hip_train(SkipCat((h, hs.pop())), emb, context, img_mask)
            saved_out.append(s)
        g, st = self.out[0].hip_train(h, silu=True)
        return self.out[2].hip(g), (saved_in, saved_mid, saved_out, h, st, context.shape)

    def hip_train_trunk(self, x_nhwc, emb, context, img_mask, n_tail):
        """hip_train without the last ``n_tail`` decoder blocks and the output head (modules/diffusionmodules/capture_graph.py):
        -> (h, [the skips those blocks will pop, in pop order], saved)."""
        self._refuse_motion("hip_train_trunk")
        self._refuse_control("hip_train_trunk")
        self._refuse_ip("hip_train_trunk")
        self._refuse_regions("hip_train_trunk")
        self._refuse_freeu("hip_train_trunk")
        saved_in, saved_out, hs = [], [], []
        h = x_nhwc
        for module in self.input_blocks:
            h, s = module.hip_train(h, emb, context, img_mask)
            saved_in.append(s)
            hs.append(h)
        h, saved_mid = self.middle_block.hip_train(h, emb, context, img_mask)
        for module in list(self.output_blocks)[:len(self.output_blocks) - n_tail]:
            h, s = module.hip_train(SkipCat((h, hs.pop())), emb, context, img_mask)
            saved_out.append(s)
        skips = [hs.pop() for _ in range(n_tail)]
        assert not hs
        return h, skips, (saved_in, saved_mid, saved_out, context.shape)

    def hip_trunk(self, x_nhwc, emb, context, img_mask, n_tail):
        """``hip_train_trunk`` for a pass that needs NO gradient below the tail (a no-grad instance of a compositional step, or one whose
        input and context carry none): the inference walk -- every cross-attention layer's k / v from one GEMM, the fused C = 320 blocks,
        nothing saved -- up to the last ``n_tail`` decoder blocks.  -> (h, [the skips those blocks pop, in pop order])."""
        self._refuse_motion("the trunk cache (hip_trunk)")
        self._refuse_control("the trunk cache (hip_trunk)")
        self._refuse_ip("the trunk cache (hip_trunk)")
        self._refuse_regions("the trunk cache (hip_trunk)")
        self._refuse_freeu("the trunk cache (hip_trunk)")
        kv_layers = self._project_context_all(context)
        try:
            hs = []
            h = x_nhwc
            for module in self.input_blocks:
                h = module.hip(h, emb, context, img_mask)
                hs.append(h)
            h = self.middle_block.hip(h, emb, context, img_mask)
            for module in list(self.output_blocks)[:len(self.output_blocks) - n_tail]:
                h = module.hip(SkipCat((h, hs.pop())), emb, context, img_mask)
            skips = [hs.pop() for _ in range(n_tail)]
            assert not hs
            return h, skips
        finally:
            for m in kv_layers:
                m._kv_pre = None

    def hip_bwd_trunk(self, saved, dh, dskips_tail, need_dx=True, res_gradscale=1.0):
        """Backward of hip_train_trunk: dh = gradient of h, dskips_tail[i] = gradient of the i-th popped skip (already scaled by the
        tail where the live path scales it) or None.  Same walk as hip_bwd."""
        self._refuse_freeu("hip_bwd_trunk")
        saved_in, saved_mid, saved_out, ctx_shape = saved
        n_in, n_out, n_tail = len(self.input_blocks), len(self.output_blocks), len(dskips_tail)
        d, dctx = dh, None
        dskips = {}
        for k, g in enumerate(dskips_tail):                      # the k-th tail block popped hs[n_tail - 1 - k]
            dskips[n_tail - 1 - k] = (g, False)
        blocks = list(self.output_blocks)[:n_out - n_tail]
        for oi in range(len(blocks) - 1, -1, -1):
            (d, dskip), dctx = blocks[oi].hip_bwd(saved_out[oi], d, dctx)
            dskips[n_in - 1 - oi] = (dskip, res_gradscale != 1.0 and oi >= self.num_res_blocks + 1)
        d, dctx = self.middle_block.hip_bwd(saved_mid, d, dctx)
        for i in range(n_in - 1, -1, -1):
            g, scaled = dskips[i]
            if g is not None:
                d = ops.axpy(d, g, res_gradscale) if scaled else ops.add(d, g)
            if i == 0 and not need_dx:
                return None, dctx.reshape(ctx_shape)
            d, dctx = self.input_blocks[i].hip_bwd(saved_in[i], d, dctx)
        return d, dctx.reshape(ctx_shape)

    def hip_bwd(self, saved, deps_nhwc, need_dx=True, res_gradscale=1.0):
        """Activation-gradient backward: deps [B,H,W,roundup(out_channels,8)] fp16 (zero padded) ->
        (dx [B,H,W,in_channels] or None, dcontext [B,L,ctx] fp16).  Skip-connection gradients from the
        decoder are added to the encoder's output gradients as the walk reaches them; `res_gradscale` multiplies the
        gradient of the skips consumed by output blocks >= num_res_blocks + 1 (the live path's
        res_hidden_states_gradscale on diffusers up_blocks[1:], diffusers_attn_lora_capture.py:382-396, 606-609)."""
        self._refuse_freeu("hip_bwd")
        saved_in, saved_mid, saved_out, h_last, st, ctx_shape = saved
        d = self.out[0].hip_bwd(h_last, st, self.out[2].hip_dgrad(deps_nhwc), silu=True)
        dctx = None
        dskips = []
        for module, s in zip(reversed(self.output_blocks), reversed(saved_out)):
            (d, dskip), dctx = module.hip_bwd(s, d, dctx)
            dskips.append(dskip)   # the LAST decoder block consumed hs[0], so this appends d(hs[0]), d(hs[1]), ...
        d, dctx = self.middle_block.hip_bwd(saved_mid, d, dctx)
        n_in = len(self.input_blocks)
        n_out = len(self.output_blocks)
        for i in range(n_in - 1, -1, -1):
            scaled = res_gradscale != 1.0 and (n_out - 1 - i) >= self.num_res_blocks + 1     # hs[i] fed output block n_out-1-i
            d = ops.axpy(d, dskips[i], res_gradscale) if scaled else ops.add(d, dskips[i])
            if i == 0 and not need_dx:
                return None, dctx.reshape(ctx_shape)
            d, dctx = self.input_blocks[i].hip_bwd(saved_in[i], d, dctx)
        return d, dctx.reshape(ctx_shape)

    def forward(self, x, timesteps=None, context=None, y=None, context_in=None, extra_info=None, **kwargs):
        """Reference contract (openaimodel.py:820-952): x [N,4,H,W], timesteps [N], context
        [N,L,ctx]; ``extra_info`` carries ``img_mask`` / ``capture_ca_activations`` in and
        receives ``ca_layers_activations`` out.  Returns eps [N,out_channels,H,W] in x.dtype."""
        assert y is None, "must specify y if and only if the model is class-conditional"
        capture = extra_info.get("capture_ca_activations", False) if extra_info is not None else False
        img_mask = extra_info.get("img_mask", None) if extra_info is not None else None
        captured = [22, 23, 24] if capture else []
        old_flags = None
        if capture:
            old_flags, _ = self.set_cross_attn_flags(ca_flag_dict={"save_cross_attn_vars": True}, ca_layer_indices=captured)
        ei = extra_info or {}
        rewrites = bool(ei.get("normalize_cross_attn", False) or ei.get("mix_attn_mats_in_batch", False))
        trainable = torch.is_grad_enabled() and (x.requires_grad or context.requires_grad or ei.get("_ffn_lora_adapters")
                                                 or ei.get("_attn_lora_adapters"))
        if rewrites or ei.get("_attn_lora_adapters") or (capture and trainable):
            # Stage-2 pass: explicit attention in the last three cross-attention layers (score rewrites, captures with gradients,
            # attention LoRAs) as a chain of autograd nodes -- modules/diffusionmodules/capture_graph.py
            from .capture_graph import unet_forward_captured
            self._refuse_motion("the captured / score-rewrite path")
            self._refuse_control("the captured / score-rewrite path")
            self._refuse_ip("the captured / score-rewrite path")
            self._refuse_regions("the captured / score-rewrite path")
            self._refuse_freeu("the captured / score-rewrite path")
            if extra_info is None:
                raise ValueError("extra_info must be a dict on the capture / score-rewrite path")
            if capture:
                self.set_cross_attn_flags(ca_flag_dict=old_flags, ca_layer_indices=captured)     # this path does its own capturing
            eps = unet_forward_captured(self, x, timesteps, context, extra_info)
            if not capture:
                extra_info.pop("ca_layers_activations", None)
            return eps
        if trainable:
            self._refuse_motion("training")
            self._refuse_control("training")
            self._refuse_ip("training")
            self._refuse_regions("training")
            self._refuse_freeu("training")
            gs = float((extra_info or {}).get("res_hidden_states_gradscale", 1) or 1)
            lora = (extra_info or {}).get("_ffn_lora_adapters")           # set by UNetWrapper when use_ffn_lora is on
            return _UNetFunction.apply(self, x, timesteps, context, img_mask, gs, lora, *[t[3] for t in lora_param_order(lora)])
        try:
            ctx = context.to(F16).contiguous()
            shared = None
            if img_mask is None and ei.get("_trunk_cache") is not None:
                from .capture_graph import cached_trunk
                shared = cached_trunk(ei, x.shape[0])
            if shared is not None:
                eps, acts = self.hip_tail(shared, timesteps, ctx, captured)      # the step's shared gradient-free trunk holds these rows
            else:
                xh = to_nhwc_f16(x, ops.round_up(self.in_channels, 8))
                eps, acts = self.hip(xh, timesteps, ctx, img_mask, captured)
        finally:
            if capture:
                self.set_cross_attn_flags(ca_flag_dict=old_flags, ca_layer_indices=captured)
        if extra_info is not None:
            extra_info["ca_layers_activations"] = {
                key: {li: acts[li][key] for li in acts} for key in ("outfeat", "attn", "attnscore", "q", "q2", "k", "v", "attn_out")
            }
        return from_nhwc_f16(eps, x.dtype, self.out_channels)


class _UNetFunction(torch.autograd.Function):
    """One autograd node for the whole U-Net: forward = UNetModel.hip_train, backward = the manual
    activation-gradient walk UNetModel.hip_bwd (gradients w.r.t. x and context; the base weights are
    frozen as in the reference, ddpm.py:4131-4132, so no weight gradients exist on this path)."""

    @staticmethod
    def forward(ctx, unet, x, timesteps, context, img_mask, res_gradscale=1.0, lora=None, *lora_params):
        """lora: {output-block index: {"conv1" | "conv2" | "conv_shortcut": DoRAConvAdapter}} or None; lora_params: the adapters'
        parameters in `lora_param_order(lora)` order (passed so that autograd routes their gradients).
        With ``unet.train_graphs`` (graphs.GraphedSegment pair, set by the trainer) the forward and the backward walk are each replayed
        as ONE hipGraph per input signature instead of ~450 / ~700 launches from Python."""
        ctx.res_gradscale = res_gradscale
        ctx.lora = lora
        ctx.need_dx, ctx.x_dtype, ctx.c_dtype = x.requires_grad, x.dtype, context.dtype

        def body(xs, ts, cs, ms):
            xh = to_nhwc_f16(xs, ops.round_up(unet.in_channels, 8))
            try:
                for bi, ads in (lora or {}).items():
                    unet.output_blocks[bi][0]._lora = ads
                eps, saved = unet.hip_train(xh, ts, cs.to(F16).contiguous(), ms)
            finally:
                for bi in (lora or {}):
                    unet.output_blocks[bi][0]._lora = None
            return from_nhwc_f16(eps, xs.dtype, unet.out_channels), saved

        graphs = getattr(unet, "train_graphs", None)
        if graphs is not None and x.is_cuda:
            ctx.key = (tuple(x.shape), tuple(context.shape), str(x.dtype), str(context.dtype), img_mask is not None, float(res_gradscale),
                       tuple(id(a) for _, _, _, a in lora_param_order(lora)), ctx.need_dx)
            # a second forward of the same signature before this node's backward (batch_student_steps=False: one student call per
            # denoising step) must not replay into the buffers this node still needs: GraphedSegment.busy -> that call runs eagerly
            from_graph = not graphs[0].busy(ctx.key) and graphs[0].entries.get(ctx.key, {}).get("state") in ("warm", "graph")
            out, ctx.saved = graphs[0].run(ctx.key, body, [x.detach(), timesteps, context.detach(), img_mask],
                                           refresh=lambda: _refresh_adapter_packs(lora))
            if not from_graph:
                ctx.key = None                # eager forward (first call of a signature, or the graph's buffers were held): its saved
                                              # activations are ordinary tensors, so its backward must not be captured / replayed either
            elif any(ctx.needs_input_grad):
                graphs[0].claim(ctx.key, ctx)
        else:
            ctx.key = None
            out, ctx.saved = body(x.detach(), timesteps, context.detach(), img_mask)
        ctx.unet = unet
        return out

    @staticmethod
    def backward(ctx, deps):
        unet = ctx.unet
        lora = ctx.lora
        saved = ctx.saved

        def body(de):
            # The backward is linear in d(eps), and loss gradients are tiny (MSE over ~16k pixels): scale d(eps) by a
            # power of two so that its largest entry is ~256 before the fp16 cast, unscale the results in fp32.  The
            # scale is computed and applied on the device (no host sync); a power of two makes it exact.
            amax = de.abs().amax().float().clamp_min(1e-30)
            scale = torch.exp2(torch.floor(torch.log2(256.0 / amax)))
            dh = to_nhwc_f16((de * scale).contiguous(), ops.round_up(unet.out_channels, 8))
            dx, dctx = unet.hip_bwd(saved, dh, need_dx=ctx.need_dx, res_gradscale=ctx.res_gradscale)
            lora_grads = []
            for bi, key, pname, p in lora_param_order(lora):
                g = saved[2][bi][0][5][4][key][pname]             # ResBlock saved -> (lora, s1, s2, ssc, grads)
                lora_grads.append((g / scale).to(p.dtype))
            gx = (from_nhwc_f16(dx, torch.float32, unet.in_channels) / scale).to(ctx.x_dtype) if dx is not None else None
            return (gx, (dctx.float() / scale).to(ctx.c_dtype)) + tuple(lora_grads)

        graphs = getattr(unet, "train_graphs", None)
        if graphs is not None and ctx.key is not None and graphs[0].entries.get(ctx.key, {}).get("state") == "graph":
            # only once the forward of this signature is itself a graph: its saved activations then sit at fixed addresses
            res = graphs[1].run(ctx.key, body, [deps.detach()])
        else:
            res = body(deps.detach())
        ctx.saved = None
        ctx.af_holds_replay = False                               # the replayed forward's buffers are free again
        return (None, res[0], None, res[1], None, None, None) + tuple(res[2:])


def _refresh_adapter_packs(lora):
    """Before a graph replay: re-derive the adapters' fp16 weight packs IN PLACE if the optimizer moved their parameters (the captured
    kernels read the packs at fixed addresses; modules/dora.py::DoRAConvAdapter._packs copies into the existing buffers)."""
    for bi in (lora or {}):
        for ad in lora[bi].values():
            ad._packs(refresh_scales=True)


def lora_param_order(lora):
    """Deterministic flattening of {block: {conv key: adapter}} -> [(block, key, parameter name, parameter)]."""
    out = []
    for bi in sorted(lora or {}):
        for key in sorted(lora[bi]):
            for pname in ("lora_A", "lora_B", "lora_magnitude_vector"):
                out.append((bi, key, pname, getattr(lora[bi][key], pname)))
    return out


def unet_param_shapes(cfg):
    """(name, shape) of every parameter of UNetModel(**cfg), without allocating them."""
    with torch.device("meta"):
        m = UNetModel(**cfg)
    return [(n, tuple(p.shape)) for n, p in m.named_parameters()]
