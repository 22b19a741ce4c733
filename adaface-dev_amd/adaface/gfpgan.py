"""GFPGAN face restoration (INTEGRATION.md "Face restoration (GFPGAN)"): GFPGANv1Clean, the architecture of ``GFPGANv1.3.pth`` /
``GFPGANv1.4.pth``, restated from TencentARC's ``gfpgan/archs/gfpganv1_clean_arch.py`` and ``stylegan2_clean_arch.py`` (restated, not pinned: no
copy of the reference and no checkpoint is available offline), the checkpoint loader and the public ``FaceRestorer``.

``GFPGANv1Clean(out_size=512, num_style_feat=512, channel_multiplier=2, num_mlp=8, narrow=1)`` carries the published parameter names, with the
v1.3 / v1.4 settings ``sft_half=True``, ``different_w=True``, ``input_is_latent=True`` fixed: a U-Net (``conv_body_first``, ``conv_body_down``,
``final_conv``, ``final_linear``, ``conv_body_up``, ``condition_scale`` / ``condition_shift``; ``toRGB`` loads and never runs) that turns the
degraded crop into one latent per decoder layer and a (scale, shift) pair per resolution, and a StyleGAN2 decoder (``stylegan_decoder``:
modulated convolutions, fixed noise, ``style_mlp`` loads and never runs) whose upper half of the channels is modulated by those pairs (SFT).
RGB in [-1, 1] in and out.

* ``forward(x)`` is the network in plain torch (NCHW, any float dtype): the CPU path and the reference of the tests.
* ``hip(crops)`` is the product path, fp16 NHWC ``[B, S, S, 8]`` (what ``ops.face_align_crop_any`` writes) -> fp16 ``[B, S, S, 8]`` with RGB in
  channels 0-2 and zeros behind them.  Every 3x3 / 1x1 runs on ``ops.conv3x3`` / ``ops.gemm``.  A modulated convolution runs as that same
  convolution on PER-SAMPLE weights ``gain * d[b,o] * W[o,t,i] * s[b,i]`` (``af_modulate_weights``, fp32 master weights, rounded to fp16 once),
  one launch per sample: the activations stay unscaled and the weight rows unit-norm, which is what fp16 wants.  ``af_style_epilogue`` adds
  noise and bias, applies LeakyReLU and the SFT, and saturates at +-65504; ``af_bilinear_up2`` is every x2 resample (with the RGB skip as its
  addend); the x0.5 resample is ``ops.sumpool2x2`` with the 1/4 folded into the weights that consume it (bilinear x0.5 with
  ``align_corners=False`` IS the 2x2 mean).  There is no torch fallback: a missing kernel is an error.
"""
import math
import re

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .face_align import estimate_similarity, load_rgb_u8

SLOPE = 0.2
SQRT2 = math.sqrt(2.0)
DEMOD_EPS = 1e-8
MAX_FACES = 16                                       # af_face_paste_affine_u8's limit
# facexlib's 512 x 512 FFHQ landmark template (left eye, right eye, nose tip, mouth corners), recalled and not pinned
FFHQ_TEMPLATE_512 = np.array([[192.98138, 239.94708], [318.90277, 240.1936], [256.63416, 314.01935], [201.26117, 371.41043],
                              [313.08905, 371.15118]], dtype=np.float64)


def ffhq_template(size):
    """The landmark template of a ``size`` x ``size`` crop."""
    return FFHQ_TEMPLATE_512 * (float(size) / 512.0)


def channel_table(narrow, channel_multiplier):
    """{resolution: channels}: ``ch(narrow)`` is the decoder's table, ``ch(narrow / 2)`` the U-Net's."""
    n, cm = narrow, channel_multiplier
    return {4: int(512 * n), 8: int(512 * n), 16: int(512 * n), 32: int(512 * n), 64: int(256 * cm * n), 128: int(128 * cm * n),
            256: int(64 * cm * n), 512: int(32 * cm * n), 1024: int(16 * cm * n)}


def _lrelu(t):
    return F.leaky_relu(t, SLOPE)


def _up2(t):
    return F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)


class ResBlock(nn.Module):
    def __init__(self, cin, cout, mode):
        super().__init__()
        assert mode in ("down", "up")
        self.mode = mode
        self.conv1 = nn.Conv2d(cin, cin, 3, 1, 1)
        self.conv2 = nn.Conv2d(cin, cout, 3, 1, 1)
        self.skip = nn.Conv2d(cin, cout, 1, bias=False)

    def resample(self, t):
        return F.interpolate(t, scale_factor=0.5 if self.mode == "down" else 2, mode="bilinear", align_corners=False)

    def forward(self, x):
        out = _lrelu(self.conv1(x))
        out = _lrelu(self.conv2(self.resample(out)))
        return out + self.skip(self.resample(x))


class ModulatedConv2d(nn.Module):
    def __init__(self, cin, cout, kernel_size, num_style_feat, demodulate=True, upsample=False):
        super().__init__()
        self.cin, self.cout, self.kernel_size, self.demodulate, self.upsample = cin, cout, kernel_size, demodulate, upsample
        self.modulation = nn.Linear(num_style_feat, cin, bias=True)
        nn.init.ones_(self.modulation.bias)
        self.weight = nn.Parameter(torch.randn(1, cout, cin, kernel_size, kernel_size) / math.sqrt(cin * kernel_size ** 2))

    def forward(self, x, style):
        b, c, h, w = x.shape
        s = self.modulation(style).view(b, 1, c, 1, 1)
        weight = self.weight * s
        if self.demodulate:
            weight = weight * torch.rsqrt(weight.pow(2).sum([2, 3, 4]) + DEMOD_EPS).view(b, self.cout, 1, 1, 1)
        weight = weight.view(b * self.cout, c, self.kernel_size, self.kernel_size)
        if self.upsample:
            x = _up2(x)
        b, c, h, w = x.shape
        out = F.conv2d(x.reshape(1, b * c, h, w), weight, padding=self.kernel_size // 2, groups=b)
        return out.view(b, self.cout, h, w)


class StyleConv(nn.Module):
    def __init__(self, cin, cout, num_style_feat, upsample=False):
        super().__init__()
        self.modulated_conv = ModulatedConv2d(cin, cout, 3, num_style_feat, demodulate=True, upsample=upsample)
        self.weight = nn.Parameter(torch.zeros(1))                  # the noise weight
        self.bias = nn.Parameter(torch.zeros(1, cout, 1, 1))

    def forward(self, x, style, noise):
        out = self.modulated_conv(x, style) * SQRT2
        return _lrelu(out + self.weight * noise + self.bias)


class ToRGB(nn.Module):
    def __init__(self, cin, num_style_feat, upsample=True):
        super().__init__()
        self.upsample = upsample
        self.modulated_conv = ModulatedConv2d(cin, 3, 1, num_style_feat, demodulate=False)
        self.bias = nn.Parameter(torch.zeros(1, 3, 1, 1))

    def forward(self, x, style, skip=None):
        out = self.modulated_conv(x, style) + self.bias
        if skip is not None:
            out = out + (_up2(skip) if self.upsample else skip)
        return out


class ConstantInput(nn.Module):
    def __init__(self, channels, size=4):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(1, channels, size, size))


class _Noises(nn.Module):
    pass


class StyleGAN2GeneratorCSFT(nn.Module):
    """StyleGAN2GeneratorClean with the SFT of the upper half of the channels between the two convolutions of a resolution."""

    def __init__(self, out_size, num_style_feat, num_mlp, channel_multiplier, narrow):
        super().__init__()
        ch = channel_table(narrow, channel_multiplier)
        layers = [nn.Identity()]                                    # NormStyleCode's slot: the linears sit at 1, 3, ...
        for _ in range(num_mlp):
            layers += [nn.Linear(num_style_feat, num_style_feat, bias=True), nn.LeakyReLU(SLOPE)]
        self.style_mlp = nn.Sequential(*layers)                     # loads; never run (the input is latent)
        self.constant_input = ConstantInput(ch[4])
        self.style_conv1 = StyleConv(ch[4], ch[4], num_style_feat)
        self.to_rgb1 = ToRGB(ch[4], num_style_feat, upsample=False)
        self.log_size = int(math.log2(out_size))
        self.num_layers = (self.log_size - 2) * 2 + 1
        self.num_latent = self.log_size * 2 - 2
        self.style_convs, self.to_rgbs, self.noises = nn.ModuleList(), nn.ModuleList(), _Noises()
        for l in range(self.num_layers):
            r = 2 ** ((l + 5) // 2)
            self.noises.register_buffer(f"noise{l}", torch.randn(1, 1, r, r))
        cin = ch[4]
        for i in range(3, self.log_size + 1):
            cout = ch[2 ** i]
            self.style_convs.append(StyleConv(cin, cout, num_style_feat, upsample=True))
            self.style_convs.append(StyleConv(cout, cout, num_style_feat))
            self.to_rgbs.append(ToRGB(cout, num_style_feat, upsample=True))
            cin = cout

    def noise(self, l):
        return getattr(self.noises, f"noise{l}")

    def forward(self, latent, conditions):
        b = latent.shape[0]
        out = self.constant_input.weight.repeat(b, 1, 1, 1)
        out = self.style_conv1(out, latent[:, 0], self.noise(0))
        skip = self.to_rgb1(out, latent[:, 1])
        i = 1
        for k in range(len(self.to_rgbs)):
            out = self.style_convs[2 * k](out, latent[:, i], self.noise(2 * k + 1))
            half = out.shape[1] // 2
            out = torch.cat([out[:, :half], out[:, half:] * conditions[i - 1] + conditions[i]], dim=1)
            out = self.style_convs[2 * k + 1](out, latent[:, i + 1], self.noise(2 * k + 2))
            skip = self.to_rgbs[k](out, latent[:, i + 2], skip)
            i += 2
        return skip


class _ModConvPack:
    """What the device walk keeps of one modulated convolution."""
    __slots__ = ("w", "wsq", "mod", "cout", "cin", "taps", "npad", "kpad", "bias", "noise", "nw")


class GFPGANv1Clean(nn.Module):
    def __init__(self, out_size=512, num_style_feat=512, channel_multiplier=2, num_mlp=8, narrow=1):
        super().__init__()
        log_size = int(round(math.log2(out_size)))
        if 2 ** log_size != out_size or not 8 <= out_size <= 1024:
            raise ValueError(f"GFPGANv1Clean out_size must be a power of two from 8 to 1024, got {out_size!r}")
        self.out_size, self.num_style_feat, self.channel_multiplier, self.num_mlp, self.narrow = out_size, num_style_feat, channel_multiplier, num_mlp, narrow
        self.log_size = log_size
        self.num_latent = 2 * log_size - 2
        U = channel_table(narrow * 0.5, channel_multiplier)
        D = channel_table(narrow, channel_multiplier)
        levels = [2 ** i for i in range(3, log_size + 1)]
        if any(U[r] < 8 or U[r] % 8 or D[r] != 2 * U[r] for r in [4] + levels) or num_style_feat % 8:
            raise ValueError(f"GFPGANv1Clean: channel counts must be multiples of 8 (and the decoder's twice the U-Net's), got U-Net "
                             f"{[U[r] for r in [4] + levels]}, decoder {[D[r] for r in [4] + levels]}, num_style_feat {num_style_feat}")
        self.unet_channels, self.decoder_channels = U, D
        self.conv_body_first = nn.Conv2d(3, U[out_size], 1)
        self.conv_body_down = nn.ModuleList()
        cin = U[out_size]
        for i in range(log_size, 2, -1):
            self.conv_body_down.append(ResBlock(cin, U[2 ** (i - 1)], "down"))
            cin = U[2 ** (i - 1)]
        self.final_conv = nn.Conv2d(cin, U[4], 3, 1, 1)
        cin = U[4]
        self.conv_body_up = nn.ModuleList()
        for r in levels:
            self.conv_body_up.append(ResBlock(cin, U[r], "up"))
            cin = U[r]
        self.toRGB = nn.ModuleList([nn.Conv2d(U[r], 3, 1) for r in levels])     # loads; never run (GFPGANer calls with return_rgb=False)
        self.final_linear = nn.Linear(U[4] * 16, self.num_latent * num_style_feat)
        self.stylegan_decoder = StyleGAN2GeneratorCSFT(out_size, num_style_feat, num_mlp, channel_multiplier, narrow)

        def cond(c):
            return nn.Sequential(nn.Conv2d(c, c, 3, 1, 1), nn.LeakyReLU(SLOPE), nn.Conv2d(c, c, 3, 1, 1))

        self.condition_scale = nn.ModuleList([cond(U[r]) for r in levels])
        self.condition_shift = nn.ModuleList([cond(U[r]) for r in levels])
        self.__dict__["_hip_cache"] = None            # (key, prepared device weights)
        self.__dict__["_hip_scratch"] = {}            # {(device, cout, cin, taps): fp16 [B, npad, kpad]} per-sample weights, grown on demand

    # ------------------------------------------------------------------ plain torch: the CPU path and the reference
    def forward(self, x):
        n = self.log_size - 2
        feat = _lrelu(self.conv_body_first(x))
        skips = []
        for i in range(n):
            feat = self.conv_body_down[i](feat)
            skips.insert(0, feat)
        feat = _lrelu(self.final_conv(feat))
        latent = self.final_linear(feat.reshape(feat.shape[0], -1)).view(feat.shape[0], self.num_latent, self.num_style_feat)
        conditions = []
        for i in range(n):
            feat = self.conv_body_up[i](feat + skips[i])
            conditions += [self.condition_scale[i](feat), self.condition_shift[i](feat)]
        return self.stylegan_decoder(latent, conditions)

    # ------------------------------------------------------------------ the HIP path
    def _prepare(self, device):
        """The weights as the kernels read them, prepared once and kept while the parameters and buffers stay what they were: the key holds
        every tensor's storage address and version counter, so loading, moving, casting or editing one in place prepares them again."""
        tensors = list(self.parameters()) + list(self.buffers())
        key = (device, tuple((p.data_ptr(), p._version) for p in tensors))
        cache = self.__dict__["_hip_cache"]
        if cache is not None and cache[0] == key:
            return cache[1]
        f32 = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()
        c = {"slope": torch.full((1,), SLOPE, dtype=torch.float32, device=device)}
        w = self.conv_body_first.weight.detach().float().reshape(-1, 3)
        c["conv_body_first"] = ops.pack_matrix(F.pad(w, (0, 5)), self.conv_body_first.bias, device)            # K = 8: the crop's padded channels
        for kind, blocks in (("down", self.conv_body_down), ("up", self.conv_body_up)):
            q = 0.25 if kind == "down" else 1.0                     # ops.sumpool2x2 sums: the mean's 1/4 goes into its two consumers
            for i, blk in enumerate(blocks):
                p = f"conv_body_{kind}.{i}."
                c[p + "conv1"] = ops.pack_conv3x3(blk.conv1.weight.detach().float(), blk.conv1.bias, device)
                c[p + "conv2"] = ops.pack_conv3x3(blk.conv2.weight.detach().float() * q, blk.conv2.bias, device)
                c[p + "skip"] = ops.pack_matrix(blk.skip.weight.detach().float().reshape(blk.skip.weight.shape[0], -1) * q, None, device)
        c["final_conv"] = ops.pack_conv3x3(self.final_conv.weight.detach().float(), self.final_conv.bias, device)
        u4 = self.unet_channels[4]
        wl = self.final_linear.weight.detach().float().view(-1, u4, 4, 4).permute(0, 2, 3, 1).reshape(-1, 16 * u4)   # columns in (y, x, c) order
        c["final_linear"] = ops.pack_matrix(wl, self.final_linear.bias, device)
        for name, seqs in (("condition_scale", self.condition_scale), ("condition_shift", self.condition_shift)):
            for i, seq in enumerate(seqs):
                for j in (0, 2):
                    c[f"{name}.{i}.{j}"] = ops.pack_conv3x3(seq[j].weight.detach().float(), seq[j].bias, device)
        dec = self.stylegan_decoder
        c["const"] = dec.constant_input.weight.detach().to(device=device, dtype=torch.float16).permute(0, 2, 3, 1).contiguous()

        def modconv(mc, bias, pad_bias_to=0):
            m = _ModConvPack()
            wt = f32(mc.weight)[0]                                 # [cout, cin, k, k]
            m.cout, m.cin, m.taps = wt.shape[0], wt.shape[1], wt.shape[2] * wt.shape[3]
            m.w = wt.permute(0, 2, 3, 1).reshape(m.cout, m.taps, m.cin).contiguous()
            m.wsq = (m.w * m.w).sum(dim=1).contiguous() if mc.demodulate else None
            m.mod = ops.pack_matrix(mc.modulation.weight.detach().float(), mc.modulation.bias, device)
            m.npad, m.kpad = ops.round_up(m.cout, 128), ops.round_up(m.taps * m.cin, 64)
            b = f32(bias).reshape(-1)
            m.bias = F.pad(b, (0, pad_bias_to - b.numel())) if pad_bias_to > b.numel() else b
            m.noise, m.nw = None, 0.0
            return m

        convs = [("style_conv1", dec.style_conv1, 0)] + [(f"style_convs.{j}", sc, j + 1) for j, sc in enumerate(dec.style_convs)]
        for name, sc, l in convs:
            m = modconv(sc.modulated_conv, sc.bias)
            m.noise, m.nw = f32(dec.noise(l)).reshape(-1), float(sc.weight.detach().float().item())
            c[name] = m
        for name, tr in [("to_rgb1", dec.to_rgb1)] + [(f"to_rgbs.{k}", t) for k, t in enumerate(dec.to_rgbs)]:
            c[name] = modconv(tr.modulated_conv, tr.bias, pad_bias_to=8)
        self.__dict__["_hip_cache"] = (key, c)
        return c

    def _weights_scratch(self, device, m, B):
        """The per-sample weight buffer of a layer shape: zeroed when allocated (af_modulate_weights writes the cout x K block only), grown
        when a larger batch arrives, reused across calls."""
        key = (device, m.cout, m.cin, m.taps)
        buf = self.__dict__["_hip_scratch"].get(key)
        if buf is None or buf.shape[0] < B:
            buf = torch.zeros((B, m.npad, m.kpad), dtype=torch.float16, device=device)
            self.__dict__["_hip_scratch"][key] = buf
        return buf[:B]

    def _modulated(self, m, latent, gain):
        styles = ops.gemm(latent, m.mod, out_f32=True)                          # fp32 [B, cin]
        return ops.modulate_weights(m.w, m.wsq, styles, self._weights_scratch(latent.device, m, latent.shape[0]), gain)

    def _style_conv(self, m, x, latent, upsample=False, sft=None):
        B = latent.shape[0]
        wt = self._modulated(m, latent, SQRT2)
        if upsample:
            x = ops.bilinear_up2(x)
        _, H, W, _ = x.shape
        y = torch.empty((B, H, W, m.cout), dtype=torch.float16, device=x.device)
        for b in range(B):                                                      # one convolution per sample: its own weights
            pw = ops.PackedWeight(wt[b], None, m.cout, m.taps * m.cin, m.kpad, 9, m.cin)
            ops.conv3x3(x[b:b + 1] if x.shape[0] > 1 else x, pw, out=y[b:b + 1])
        scale, shift = sft if sft is not None else (None, None)
        return ops.style_epilogue(y, m.noise, m.bias, scale, shift, nw=m.nw, out=y)

    def _to_rgb(self, m, x, latent, skip):
        B, H, W, cin = x.shape
        wt = self._modulated(m, latent, 1.0)
        rgb = torch.empty((B, H, W, 8), dtype=torch.float16, device=x.device)
        for b in range(B):
            pw = ops.PackedWeight(wt[b], m.bias, 8, cin, m.kpad, 1, cin)         # rows 3 .. 7 are the buffer's zeros: channels 3 .. 7 come out 0
            ops.gemm(x[b].view(H * W, cin), pw, out=rgb[b].view(H * W, 8))
        return rgb if skip is None else ops.bilinear_up2(skip, addend=rgb)

    @torch.no_grad()
    def hip(self, crops):
        S = self.out_size
        if (not torch.is_tensor(crops) or crops.dtype != torch.float16 or crops.dim() != 4 or tuple(crops.shape[1:]) != (S, S, 8)
                or not crops.is_cuda or crops.shape[0] < 1):
            raise RuntimeError(f"GFPGANv1Clean.hip: expected a non-empty fp16 device tensor [B, {S}, {S}, 8] (ops.face_align_crop_any), got "
                               f"{tuple(crops.shape) if torch.is_tensor(crops) else type(crops).__name__}")
        B = crops.shape[0]
        U, D = self.unet_channels, self.decoder_channels
        widest = max(max(U[r], D[r]) * r * r for r in [2 ** i for i in range(2, self.log_size + 1)])
        if B * widest >= 2 ** 31:
            raise ValueError(f"{B} crops of {S} x {S} need a tensor of 2^31 elements or more: restore them in smaller batches")
        crops = crops.contiguous()
        c = self._prepare(crops.device)
        n = self.log_size - 2
        lrelu = lambda t: ops.affine_prelu(t, slope=c["slope"])
        feat = lrelu(ops.gemm(crops.view(B * S * S, 8), c["conv_body_first"])).view(B, S, S, -1)
        skips = []
        for i in range(n):
            p = f"conv_body_down.{i}."
            t = ops.sumpool2x2(lrelu(ops.conv3x3(feat, c[p + "conv1"])))
            o = lrelu(ops.conv3x3(t, c[p + "conv2"]))
            xp = ops.sumpool2x2(feat)
            feat = ops.gemm(xp.view(-1, xp.shape[3]), c[p + "skip"], residual=o.view(-1, o.shape[3])).view(o.shape)
            skips.insert(0, feat)
        feat = lrelu(ops.conv3x3(feat, c["final_conv"]))
        latent = ops.gemm(feat.view(B, -1), c["final_linear"]).view(B, self.num_latent, self.num_style_feat)
        latent = latent.transpose(0, 1).contiguous()                            # [L, B, nsf]: latent[i] is the A operand of layer i's modulation
        conds = []
        for i in range(n):
            p = f"conv_body_up.{i}."
            feat = ops.add(feat, skips[i])
            t = ops.bilinear_up2(lrelu(ops.conv3x3(feat, c[p + "conv1"])))
            o = lrelu(ops.conv3x3(t, c[p + "conv2"]))
            xu = ops.bilinear_up2(feat)
            feat = ops.gemm(xu.view(-1, xu.shape[3]), c[p + "skip"], residual=o.view(-1, o.shape[3])).view(o.shape)
            conds.append(tuple(ops.conv3x3(lrelu(ops.conv3x3(feat, c[f"{name}.{i}.0"])), c[f"{name}.{i}.2"])
                               for name in ("condition_scale", "condition_shift")))
        del skips
        out = self._style_conv(c["style_conv1"], c["const"], latent[0])
        skip = self._to_rgb(c["to_rgb1"], out, latent[1], None)
        j = 1
        for k in range(n):
            out = self._style_conv(c[f"style_convs.{2 * k}"], out, latent[j], upsample=True, sft=conds[k])
            out = self._style_conv(c[f"style_convs.{2 * k + 1}"], out, latent[j + 1])
            skip = self._to_rgb(c[f"to_rgbs.{k}"], out, latent[j + 2], skip)
            j += 2
        return skip


def expected_keys(out_size=512, num_style_feat=512, channel_multiplier=2, narrow=1, num_mlp=8):
    """{state-dict key: shape} of the published GFPGANv1Clean layout (sft_half, different_w): 285 entries at the v1.4 configuration."""
    log_size = int(round(math.log2(out_size)))
    U, D = channel_table(narrow * 0.5, channel_multiplier), channel_table(narrow, channel_multiplier)
    nsf = num_style_feat
    keys = {}

    def conv(name, cout, cin, k, bias=True):
        keys[name + ".weight"] = (cout, cin, k, k)
        if bias:
            keys[name + ".bias"] = (cout,)

    def res(name, cin, cout):
        conv(name + ".conv1", cin, cin, 3)
        conv(name + ".conv2", cout, cin, 3)
        conv(name + ".skip", cout, cin, 1, bias=False)

    def modconv(name, cout, cin, k):
        keys[name + ".modulated_conv.weight"] = (1, cout, cin, k, k)
        keys[name + ".modulated_conv.modulation.weight"] = (cin, nsf)
        keys[name + ".modulated_conv.modulation.bias"] = (cin,)

    def style_conv(name, cin, cout):
        modconv(name, cout, cin, 3)
        keys[name + ".weight"], keys[name + ".bias"] = (1,), (1, cout, 1, 1)

    def to_rgb(name, cin):
        modconv(name, 3, cin, 1)
        keys[name + ".bias"] = (1, 3, 1, 1)

    conv("conv_body_first", U[out_size], 3, 1)
    cin = U[out_size]
    for j, i in enumerate(range(log_size, 2, -1)):
        res(f"conv_body_down.{j}", cin, U[2 ** (i - 1)])
        cin = U[2 ** (i - 1)]
    conv("final_conv", U[4], cin, 3)
    keys["final_linear.weight"], keys["final_linear.bias"] = ((2 * log_size - 2) * nsf, U[4] * 16), ((2 * log_size - 2) * nsf,)
    cin = U[4]
    for j, i in enumerate(range(3, log_size + 1)):
        c = U[2 ** i]
        res(f"conv_body_up.{j}", cin, c)
        conv(f"toRGB.{j}", 3, c, 1)
        for name in ("condition_scale", "condition_shift"):
            conv(f"{name}.{j}.0", c, c, 3)
            conv(f"{name}.{j}.2", c, c, 3)
        cin = c
    d = "stylegan_decoder."
    for i in range(num_mlp):
        keys[f"{d}style_mlp.{2 * i + 1}.weight"], keys[f"{d}style_mlp.{2 * i + 1}.bias"] = (nsf, nsf), (nsf,)
    keys[d + "constant_input.weight"] = (1, D[4], 4, 4)
    style_conv(d + "style_conv1", D[4], D[4])
    to_rgb(d + "to_rgb1", D[4])
    cin = D[4]
    for j, i in enumerate(range(3, log_size + 1)):
        c = D[2 ** i]
        style_conv(f"{d}style_convs.{2 * j}", cin, c)
        style_conv(f"{d}style_convs.{2 * j + 1}", c, c)
        to_rgb(f"{d}to_rgbs.{j}", c)
        cin = c
    for l in range((log_size - 2) * 2 + 1):
        r = 2 ** ((l + 5) // 2)
        keys[f"{d}noises.noise{l}"] = (1, 1, r, r)
    return keys


def infer_config(sd):
    """(out_size, num_style_feat, channel_multiplier, narrow) from the tensor shapes of a GFPGANv1Clean state dict; ValueError with a
    message for any other layout (GFPGAN v1 with its fused activations, sft_half=False, different_w=False)."""
    def shape(k):
        t = sd.get(k)
        if not torch.is_tensor(t):
            raise ValueError(f"not a GFPGANv1Clean state dict: missing key {k}" + (" (GFPGAN v1, the non-clean architecture, is not built)"
                                                                                  if any(x.startswith("conv_body_first.0.") for x in sd) else ""))
        return tuple(t.shape)

    shape("conv_body_first.weight")
    downs = [int(m.group(1)) for m in (re.match(r"conv_body_down\.(\d+)\.", k) for k in sd) if m]
    if not downs:
        raise ValueError("not a GFPGANv1Clean state dict: missing key conv_body_down.0.conv1.weight")
    out_size = 2 ** (max(downs) + 3)
    mod = shape("stylegan_decoder.style_conv1.modulated_conv.modulation.weight")
    if len(mod) != 2 or (mod[0] % 512 != 0 and 512 % mod[0] != 0):          # narrow is a multiple or a power-of-two fraction of 1
        raise ValueError(f"stylegan_decoder.style_conv1.modulated_conv.modulation.weight has shape {mod}: expected [512 narrow, num_style_feat]")
    nsf, narrow = mod[1], mod[0] / 512.0
    if narrow == int(narrow):
        narrow = int(narrow)
    cm = 2
    if out_size >= 64:
        d64 = shape("stylegan_decoder.style_convs.6.modulated_conv.weight")[1]       # the first convolution of the 64 x 64 level
        cm = d64 / (256.0 * narrow)
        if cm != int(cm) or cm < 1:
            raise ValueError(f"the decoder has {d64} channels at 64 x 64 and {mod[0]} at 4 x 4: no integer channel_multiplier fits")
        cm = int(cm)
    fl = shape("final_linear.weight")
    if fl[0] == nsf:
        raise ValueError("final_linear gives one latent for all layers (different_w=False): only the v1.3 / v1.4 layout (different_w=True) is built")
    cs = shape("condition_scale.0.2.weight")
    if cs[0] == 2 * cs[1]:
        raise ValueError("condition_scale modulates every channel (sft_half=False): only the v1.3 / v1.4 layout (sft_half=True) is built")
    return out_size, nsf, cm, narrow


def load_gfpgan(path_or_state_dict):
    """A GFPGANv1Clean from a local ``.pth`` file or a state dict (``params_ema`` / ``params`` wrappers are unwrapped).  ``out_size``,
    ``num_style_feat``, ``channel_multiplier`` and ``narrow`` come from tensor shapes (a network below 64 pixels does not show its
    channel_multiplier: 2 is taken).  Strict: missing, unexpected or mis-shaped keys raise ValueError naming them.  Nothing is downloaded."""
    sd = path_or_state_dict
    if not isinstance(sd, dict):
        sd = torch.load(str(sd), map_location="cpu", weights_only=True)
    for wrap in ("params_ema", "params"):
        if wrap in sd and isinstance(sd[wrap], dict):
            sd = sd[wrap]
            break
    out_size, nsf, cm, narrow = infer_config(sd)
    want = expected_keys(out_size, nsf, cm, narrow)
    missing = sorted(k for k in want if k not in sd)
    unexpected = sorted(k for k in sd if k not in want)
    bad = sorted(f"{k} {tuple(sd[k].shape)} (expected {want[k]})" for k in want if k in sd and tuple(sd[k].shape) != want[k])
    if missing or unexpected or bad:
        parts = [f"{n}: {', '.join(v[:8])}{' ...' if len(v) > 8 else ''}" for n, v in (("missing keys", missing), ("unexpected keys", unexpected),
                                                                                      ("mis-shaped keys", bad)) if v]
        raise ValueError(f"the state dict does not match GFPGANv1Clean (out_size {out_size}, num_style_feat {nsf}, channel_multiplier {cm}, "
                         f"narrow {narrow}) -- " + "; ".join(parts))
    net = GFPGANv1Clean(out_size, nsf, cm, 8, narrow)
    net.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return net.eval()


class FaceRestorer:
    """The public object.  ``restorer(images)`` takes a path, a PIL image, a uint8 array or tensor ``[H, W, 3]`` (or a list of them) and returns
    the restored image(s): a PIL image for a path or a PIL image, otherwise the kind that came in.  Every face ``detect_faces`` finds
    (``FaceIDExtractor``'s contract: ``detect_faces(rgb_u8) -> [(x, y, w, h, confidence, kps[5][2]), ...]``; a ``RetinaFaceDetector`` fits), at
    most ``max_faces`` in the detector's order (or the one nearest the centre with ``only_center_face``), is aligned onto the FFHQ template at
    the network's size by the tree's least-squares similarity, restored in one batch, and pasted back by one launch with a soft border:
    alpha rises from 0 at ``erode`` (a fraction of the crop size) inside the crop's edge to 1 over ``feather``.  An image without a face comes
    back unchanged."""

    def __init__(self, net, detect_faces, device="cuda", erode=0.05, feather=0.10, max_faces=MAX_FACES, only_center_face=False):
        if not isinstance(net, GFPGANv1Clean):
            raise ValueError(f"FaceRestorer takes a GFPGANv1Clean (see load_gfpgan), got {type(net).__name__}")
        if not callable(detect_faces):
            raise ValueError("FaceRestorer needs detect_faces, a callable with FaceIDExtractor's detector contract")
        if not (erode >= 0 and feather >= 0 and erode + feather < 0.5):
            raise ValueError(f"erode and feather are non-negative fractions of the crop size with erode + feather < 0.5, got {erode!r}, {feather!r}")
        if not 1 <= int(max_faces) <= MAX_FACES:
            raise ValueError(f"max_faces must be from 1 to {MAX_FACES}, got {max_faces!r}")
        self.net = net.eval()
        self.detect_faces = detect_faces
        self.device = device
        self.erode, self.feather, self.max_faces, self.only_center_face = float(erode), float(feather), int(max_faces), bool(only_center_face)
        self.size = net.out_size

    def face_matrices(self, rgb):
        """Host: (forward [F, 2, 3] image -> crop, inverse [F, 2, 3] crop -> image) as fp32 arrays, F = 0 without a face."""
        faces = [f for f in (self.detect_faces(rgb) or []) if len(f) > 5 and f[5] is not None]
        if self.only_center_face and faces:
            H, W = rgb.shape[:2]
            faces = [min(faces, key=lambda f: (f[0] + f[2] / 2 - W / 2) ** 2 + (f[1] + f[3] / 2 - H / 2) ** 2)]
        faces = faces[:self.max_faces]
        template = ffhq_template(self.size)
        mats = [estimate_similarity(f[5], template) for f in faces]
        fwd = np.stack([m[0] for m in mats]).astype(np.float32) if mats else np.zeros((0, 2, 3), dtype=np.float32)
        inv = np.stack([m[1] for m in mats]).astype(np.float32) if mats else np.zeros((0, 2, 3), dtype=np.float32)
        return fwd, inv

    def restore_u8(self, photo_u8):
        """uint8 [H, W, 3] on any device -> uint8 [H, W, 3] on ``self.device`` (the input itself, moved, when no face is found)."""
        if not torch.is_tensor(photo_u8) or photo_u8.dtype != torch.uint8 or photo_u8.dim() != 3 or photo_u8.shape[2] != 3 or photo_u8.numel() == 0:
            raise ValueError("the face restorer takes a non-empty uint8 tensor [H, W, 3]")
        if photo_u8.numel() >= 1 << 31:
            raise ValueError(f"the photo needs 2^31 bytes or more ({photo_u8.shape[1]} x {photo_u8.shape[0]}): the kernels use 32-bit offsets")
        fwd, inv = self.face_matrices(np.ascontiguousarray(photo_u8.cpu().numpy()))
        photo = photo_u8.to(self.device).contiguous()
        if not len(fwd):
            return photo
        if next(self.net.parameters()).device.type != torch.device(self.device).type:
            self.net.to(self.device)                 # once: moving the network drops its prepared device weights
        crops = ops.face_align_crop_any(photo, torch.from_numpy(inv).to(photo.device), self.size)
        restored = self.net.hip(crops)
        return ops.face_paste_affine_u8(photo, restored, torch.from_numpy(fwd).to(photo.device), self.erode * self.size, self.feather * self.size)

    def __call__(self, images):
        from PIL import Image
        if isinstance(images, (list, tuple)):
            return [self(im) for im in images]
        if torch.is_tensor(images):
            return self.restore_u8(images).to(images.device)
        out = self.restore_u8(torch.from_numpy(load_rgb_u8(images))).cpu().numpy()
        return out if isinstance(images, np.ndarray) else Image.fromarray(out)
