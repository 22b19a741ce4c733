"""AnimateDiff motion modules on the SD-1.5 U-Net, inference only (INTEGRATION.md "Video (motion modules)").

Restated from AnimateDiff's ``animatediff/models/motion_module.py`` (VanillaTemporalModule -> TemporalTransformer3DModel ->
TemporalTransformerBlock with two "Temporal_Self" VersatileAttention layers and a GEGLU feed-forward) and its U-Net placement; the contract
is NOT pinned against a reference copy (none is available offline), parameter names follow the published ``mm_sd_v14`` / ``v15`` / ``v15_v2``
checkpoints.

A ``TemporalTransformer`` works on the U-Net's NHWC activation ``x [B*F, H, W, C]`` (video-major: row ``v*F + f``) without rearranging it:

    h = proj_in(GroupNorm(x))                                    af_groupnorm, af_gemm
    for k in 0, 1:  h += to_out_k(Attn(LN_k(h) + pe[f]))         q|k|v: ONE af_gemm with LN_k folded in (ops.pack_matrix_ln) and W_qkv pe[f] as
                                                                 its per-image row bias (W (LN(h) + pe_f) = W LN(h) + W pe_f); the attention over
                                                                 the frames of each pixel: af_temporal_attention; to_out: af_gemm + residual
    h += ff(LN(h))                                               FeedForward.hip with its folded LayerNorm
    y = x + proj_out(h)                                          af_gemm with residual = x
"""
import math

import torch
import torch.nn as nn

from ... import ops
from .attention import FeedForward, Normalize, ln_fold
from .diffusionmodules.util import LayerNorm, Linear, _PackCache

MAX_FRAMES = ops.TEMPORAL_ATTN_MAX_FRAMES


def sinusoidal_pe(max_len: int, channels: int) -> torch.Tensor:
    """AnimateDiff's PositionalEncoding table [1, max_len, C]: pe[pos, 2i] = sin(pos * exp(-2i ln(10000) / C)), pe[pos, 2i+1] the cosine."""
    pos = torch.arange(max_len, dtype=torch.float64)[:, None]
    div = torch.exp(torch.arange(0, channels, 2, dtype=torch.float64) * (-math.log(10000.0) / channels))
    pe = torch.zeros(1, max_len, channels, dtype=torch.float64)
    pe[0, :, 0::2] = torch.sin(pos * div)
    pe[0, :, 1::2] = torch.cos(pos * div)[:, :channels // 2]
    return pe.float()


class _PosEncoder(nn.Module):
    def __init__(self, channels, max_len):
        super().__init__()
        self.register_buffer("pe", sinusoidal_pe(max_len, channels))


class TemporalAttention(nn.Module):
    """One "Temporal_Self" attention: q, k and v all come from LN(h) + pe[f]; softmax over the frames of each pixel, scale d^-0.5."""

    def __init__(self, channels, heads, max_len):
        super().__init__()
        if channels % heads or (channels // heads) % 8 or not 8 <= channels // heads <= 160:
            raise ValueError(f"TemporalAttention: {channels} channels over {heads} heads: the head dim must be a multiple of 8 in 8 .. 160")
        self.heads, self.dim_head = heads, channels // heads
        self.to_q = Linear(channels, channels, bias=False)
        self.to_k = Linear(channels, channels, bias=False)
        self.to_v = Linear(channels, channels, bias=False)
        self.to_out = nn.Sequential(Linear(channels, channels))
        self.pos_encoder = _PosEncoder(channels, max_len)
        self._qkv_cache, self._qkv_cache_ln, self._pe_cache = _PackCache(), _PackCache(), _PackCache()
        self._pe_rows = {}

    def _weights(self):
        return (self.to_q.weight, self.to_k.weight, self.to_v.weight)

    def _packed_qkv(self, ln):
        ws = self._weights()
        if ln is None:
            return self._qkv_cache.get(ws, lambda: ops.pack_matrix(torch.cat([w.detach() for w in ws], 0), None, ws[0].device))
        return self._qkv_cache_ln.get(ws + (ln.weight, ln.bias), lambda: ops.pack_matrix_ln(
            torch.cat([w.detach() for w in ws], 0), None, ln.weight, ln.bias, ln.eps, ws[0].device))

    def _pe_rowbias(self, B, F):
        """W_qkv pe[f] for f < F, repeated per video: fp16 [B*F, 3C], the row bias of the q|k|v GEMM (one row per image)."""
        ws = self._weights()

        def build():
            self._pe_rows = {}
            w = torch.cat([p.detach().float().cpu() for p in ws], 0)                  # one-off, on the host: [3C, C]
            return (self.pos_encoder.pe[0].detach().float().cpu() @ w.t()).to(device=ws[0].device, dtype=ops.F16)

        table = self._pe_cache.get(ws + (self.pos_encoder.pe,), build)
        rows = self._pe_rows.get((B, F))
        if rows is None:
            rows = self._pe_rows[(B, F)] = table[:F].repeat(B, 1).contiguous()
        return rows

    def hip(self, h, ln, B, F, HW):
        """h [B*F*HW, C] fp16 (un-normalised) -> h + to_out(attention)."""
        fold = ln_fold(h.shape[1], h.shape[0])
        qkv = ops.gemm(h if fold else ln.hip(h), self._packed_qkv(ln if fold else None), rowbias=self._pe_rowbias(B, F), rows_per_batch=HW)
        o = ops.temporal_attention(qkv, B=B, F=F, HW=HW, heads=self.heads, d=self.dim_head, scale=self.dim_head ** -0.5)
        return self.to_out[0].hip(o, residual=h)


class TemporalTransformerBlock(nn.Module):
    def __init__(self, channels, heads, max_len):
        super().__init__()
        self.attention_blocks = nn.ModuleList([TemporalAttention(channels, heads, max_len) for _ in range(2)])
        self.norms = nn.ModuleList([LayerNorm(channels) for _ in range(2)])
        self.ff = FeedForward(channels, glu=True)
        self.ff_norm = LayerNorm(channels)

    def hip(self, h, B, F, HW):
        for attn, ln in zip(self.attention_blocks, self.norms):
            h = attn.hip(h, ln, B, F, HW)
        ln = self.ff_norm if ln_fold(h.shape[1]) else None
        return self.ff.hip(h if ln else self.ff_norm.hip(h), residual=h, ln=ln)


class TemporalTransformer(nn.Module):
    def __init__(self, channels, heads=8, max_len=32):
        super().__init__()
        if not 1 <= max_len <= MAX_FRAMES:
            raise ValueError(f"TemporalTransformer: max_len must be in 1 .. {MAX_FRAMES}, got {max_len}")
        self.channels, self.heads, self.max_len = channels, heads, max_len
        self.norm = Normalize(channels)
        self.proj_in = Linear(channels, channels)
        self.transformer_blocks = nn.ModuleList([TemporalTransformerBlock(channels, heads, max_len)])
        self.proj_out = Linear(channels, channels)

    def hip(self, x, num_frames):
        """x [B*F, H, W, C] fp16 NHWC, video-major -> same shape."""
        BF, H, W, Cn = x.shape
        F = int(num_frames)
        if not 1 <= F <= self.max_len or BF % F or Cn != self.channels:
            raise ValueError(f"TemporalTransformer: {BF} images of {Cn} channels, {F} frames: the batch must be whole videos of 1 .. "
                             f"{self.max_len} frames at {self.channels} channels")
        B, HW = BF // F, H * W
        x2d = x.reshape(BF * HW, Cn)
        h = self.proj_in.hip(self.norm.hip(x).reshape(BF * HW, Cn))
        for block in self.transformer_blocks:
            h = block.hip(h, B, F, HW)
        # as SpatialTransformer.hip: the output feeds a GroupNorm(32), so the launch leaves its partial statistics with it where it can
        out = ops.gemm(h, self.proj_out.packed(), residual=x2d, rows_per_batch=HW, gn_cpg=Cn // 32 if Cn % 32 == 0 else 0)
        out4 = out.reshape(BF, H, W, Cn)
        if hasattr(out, "_gn_partials"):
            out4._gn_partials = out._gn_partials
        return out4


# ---- placement in the LDM block numbering -----------------------------------------------------------------------------------------------
def motion_placement(with_mid=True):
    """{key prefix: (where, block index)}: ("input", n) = after input_blocks[n]; ("middle", 1) = between middle_block[1] and [2];
    ("output", n) = in output_blocks[n] behind its ResBlock and SpatialTransformer, in front of its Upsample."""
    table = {}
    for i in range(4):
        for j in range(2):
            table[f"down_blocks.{i}.motion_modules.{j}"] = ("input", 3 * i + 1 + j)
    if with_mid:
        table["mid_block.motion_modules.0"] = ("middle", 1)
    for i in range(4):
        for j in range(3):
            table[f"up_blocks.{i}.motion_modules.{j}"] = ("output", 3 * i + j)
    return table


def _read_state_dict(src):
    if isinstance(src, dict):
        sd = src
    else:
        sd = torch.load(src, map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}


class MotionModule(nn.Module):
    """The 20 (v1) or 21 (v2: + mid_block) temporal transformers of an AnimateDiff motion module, from a ``.ckpt`` / ``.pth`` file or a state
    dict.  Loading is strict: missing, unexpected or mis-shaped keys raise ValueError naming them (``pos_encoder.pe`` may be absent: it is then
    computed).  ``at(where, n)`` is the transformer placed there, or None."""

    def __init__(self, path_or_state_dict, heads=8):
        super().__init__()
        sd = _read_state_dict(path_or_state_dict)
        infix = ".temporal_transformer."
        with_mid = any(k.startswith("mid_block.") for k in sd)
        table = motion_placement(with_mid)
        unexpected = sorted(k for k in sd if infix not in k or k.split(infix)[0] not in table)
        pes = [v.shape[1] for k, v in sd.items() if k.endswith("pos_encoder.pe") and torch.is_tensor(v) and v.dim() == 3]
        if pes and (min(pes) != max(pes) or not 1 <= pes[0] <= MAX_FRAMES):
            raise ValueError(f"motion module: pos_encoder.pe lengths {sorted(set(pes))}: one length in 1 .. {MAX_FRAMES} expected")
        self.max_len = pes[0] if pes else MAX_FRAMES
        self.with_mid = with_mid
        self.transformers = nn.ModuleDict()
        self._where = {}
        missing, misshaped = [], []
        for prefix, where in table.items():
            nw = sd.get(prefix + infix + "norm.weight")
            if not torch.is_tensor(nw) or nw.dim() != 1:
                missing.append(prefix + infix + "norm.weight")
                continue
            tt = TemporalTransformer(int(nw.shape[0]), heads, self.max_len)
            own = tt.state_dict()
            sub = {k[len(prefix + infix):]: v for k, v in sd.items() if k.startswith(prefix + infix)}
            for k, v in own.items():
                if k not in sub:
                    if not k.endswith("pos_encoder.pe"):
                        missing.append(prefix + infix + k)
                elif tuple(sub[k].shape) != tuple(v.shape):
                    misshaped.append(f"{prefix + infix + k} {tuple(sub[k].shape)} (expected {tuple(v.shape)})")
            unexpected += sorted(prefix + infix + k for k in sub if k not in own)
            if not (missing or misshaped or unexpected):
                tt.load_state_dict({k: sub.get(k, v).float() for k, v in own.items()}, strict=True)
            name = prefix.replace(".", "_")
            self.transformers[name] = tt
            self._where[where] = name
        if missing or unexpected or misshaped:
            raise ValueError("motion module state dict does not match"
                             + (f"; missing: {missing}" if missing else "")
                             + (f"; unexpected: {unexpected}" if unexpected else "")
                             + (f"; wrong shape: {misshaped}" if misshaped else ""))
        self.eval().requires_grad_(False)

    def at(self, where, n):
        name = self._where.get((where, n))
        return None if name is None else self.transformers[name]

    def placed(self):
        """[((where, n), TemporalTransformer)] for every transformer."""
        return [(w, self.transformers[name]) for w, name in self._where.items()]
