"""Real-ESRGAN upscaling (INTEGRATION.md "Upscaling (Real-ESRGAN)"): RRDBNet restated from xinntao's ``basicsr/archs/rrdbnet_arch.py``
(restated, not pinned: no copy of the reference is available offline), the checkpoint loader and the public ``Upscaler``.

``RRDBNet(num_in_ch=3, num_out_ch=3, scale=4, num_feat=64, num_block=23, num_grow_ch=32)`` carries the published parameter names
(``conv_first``, ``body.{i}.rdb{1,2,3}.conv{1..5}``, ``conv_body``, ``conv_up1``, ``conv_up2``, ``conv_hr``, ``conv_last``; all 3 x 3, padding 1,
with a bias), so ``RealESRGAN_x4plus``, ``RealESRGAN_x2plus`` and ``RealESRGAN_x4plus_anime_6B`` load strictly.  RGB in [0, 1] in and out; the
output is always 4 x the convolved grid, i.e. x4, x2 (pixel_unshuffle 2 in front) or x1 (pixel_unshuffle 4) of the input image.

* ``forward(x)`` is the network in plain torch (fp32 NCHW): the CPU path and the reference of the tests.
* ``hip(images_u8)`` is the product path, uint8 ``[B, H, W, 3]`` -> uint8 ``[B, sH, sW, 3]`` on the device: ``af_u8_unshuffle_f16`` and then one
  ``af_dense_conv3x3`` launch per convolution (csrc/af_esrgan.hip).  Three rotating ``[B, H, W, 192]`` fp16 buffers, and a fourth that
  ``conv_first`` writes and that keeps its output for ``conv_body``'s residual, hold the dense blocks: an
  RDB's ``conv1..4`` write channels [64, 96) .. [160, 192) of the buffer they read, so no concatenation is ever copied; ``conv5`` writes
  channels [0, 64) of the next buffer with the block input as fused residual (and, on ``rdb3``, the RRDB input as a second one); ``conv_up1/2``
  read their input nearest-x2 upsampled without materialising it; ``conv_last`` quantises to uint8 in its epilogue.  There is no torch fallback:
  a missing kernel is an error.
"""
import re

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops

SLOPE = 0.2
RES_SCALE = 0.2
MAX_INPUT_SIDE = 1024
_UNSHUFFLE = {4: 1, 2: 2, 1: 4}                      # network scale -> pixel_unshuffle factor in front of conv_first
_SCALE_OF_IN_CH = {3: 4, 12: 2, 48: 1}


class ResidualDenseBlock(nn.Module):
    def __init__(self, num_feat=64, num_grow_ch=32):
        super().__init__()
        for k in range(1, 5):
            setattr(self, f"conv{k}", nn.Conv2d(num_feat + (k - 1) * num_grow_ch, num_grow_ch, 3, 1, 1))
        self.conv5 = nn.Conv2d(num_feat + 4 * num_grow_ch, num_feat, 3, 1, 1)

    def forward(self, x):
        x1 = F.leaky_relu(self.conv1(x), SLOPE)
        x2 = F.leaky_relu(self.conv2(torch.cat((x, x1), 1)), SLOPE)
        x3 = F.leaky_relu(self.conv3(torch.cat((x, x1, x2), 1)), SLOPE)
        x4 = F.leaky_relu(self.conv4(torch.cat((x, x1, x2, x3), 1)), SLOPE)
        x5 = self.conv5(torch.cat((x, x1, x2, x3, x4), 1))
        return x5 * RES_SCALE + x


class RRDB(nn.Module):
    def __init__(self, num_feat=64, num_grow_ch=32):
        super().__init__()
        self.rdb1 = ResidualDenseBlock(num_feat, num_grow_ch)
        self.rdb2 = ResidualDenseBlock(num_feat, num_grow_ch)
        self.rdb3 = ResidualDenseBlock(num_feat, num_grow_ch)

    def forward(self, x):
        return self.rdb3(self.rdb2(self.rdb1(x))) * RES_SCALE + x


class RRDBNet(nn.Module):
    def __init__(self, num_in_ch=3, num_out_ch=3, scale=4, num_feat=64, num_block=23, num_grow_ch=32):
        super().__init__()
        if scale not in _UNSHUFFLE:
            raise ValueError(f"RRDBNet scale must be 4, 2 or 1, got {scale!r}")
        self.scale, self.num_in_ch, self.num_out_ch, self.num_feat, self.num_grow_ch = scale, num_in_ch, num_out_ch, num_feat, num_grow_ch
        self.unshuffle = _UNSHUFFLE[scale]
        self.conv_first = nn.Conv2d(num_in_ch * self.unshuffle ** 2, num_feat, 3, 1, 1)
        self.body = nn.Sequential(*[RRDB(num_feat, num_grow_ch) for _ in range(num_block)])
        self.conv_body = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_up1 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_up2 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_hr = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_last = nn.Conv2d(num_feat, num_out_ch, 3, 1, 1)
        self.__dict__["_hip_cache"] = None            # (key, {conv name: (fp16 weights as the kernel reads them, fp32 bias)})

    # ------------------------------------------------------------------ plain torch: the CPU path and the reference
    def forward(self, x):
        f = F.pixel_unshuffle(x, self.unshuffle) if self.unshuffle > 1 else x
        f = self.conv_first(f)
        f = f + self.conv_body(self.body(f))
        f = F.leaky_relu(self.conv_up1(F.interpolate(f, scale_factor=2, mode="nearest")), SLOPE)
        f = F.leaky_relu(self.conv_up2(F.interpolate(f, scale_factor=2, mode="nearest")), SLOPE)
        return self.conv_last(F.leaky_relu(self.conv_hr(f), SLOPE))

    # ------------------------------------------------------------------ the HIP path
    def check_hip_widths(self):
        if (self.num_in_ch, self.num_out_ch, self.num_feat, self.num_grow_ch) != (3, 3, 64, 32):
            raise ValueError(f"RRDBNet.hip runs 3 -> 3 channel networks of width 64 with growth 32 (af_dense_conv3x3's dense-block layout), got "
                             f"in {self.num_in_ch}, out {self.num_out_ch}, num_feat {self.num_feat}, num_grow_ch {self.num_grow_ch}")

    def _hip_weights(self, device):
        """The convolutions' weights as af_dense_conv3x3 reads them, prepared once and kept while the parameters stay what they were: the key
        holds every parameter's storage address and version counter, so loading, moving, casting or editing a parameter in place prepares them
        again."""
        key = (device, tuple((p.data_ptr(), p._version) for p in self.parameters()))
        cache = self.__dict__["_hip_cache"]
        if cache is not None and cache[0] == key:
            return cache[1]
        cpad = self.hip_cpad
        w = {}
        for name, m in self.named_modules():
            if isinstance(m, nn.Conv2d):
                wt = ops.dense_conv3x3_weight(m.weight.detach().to(device), cpad if name == "conv_first" else None)
                w[name] = (wt, m.bias.detach().to(device=device, dtype=torch.float32).contiguous())
        self.__dict__["_hip_cache"] = (key, w)
        return w

    @property
    def hip_cpad(self):
        """Channels of conv_first's (zero-padded) input: 32 for x4 (3) and x2 (12), 64 for x1 (48)."""
        return 32 if 3 * self.unshuffle ** 2 <= 32 else 64

    def hip_batch_slice(self, H, W):
        """Images per af_dense_conv3x3 call for inputs of H x W: the widest tensors, [b, H/r, W/r, 192] in the body and [b, 4H/r, 4W/r, 64]
        in the tail, stay below the kernel's 2^31-element guard."""
        r = self.unshuffle
        return max(1, (2 ** 31 - 1) // ((H // r) * (W // r) * 16 * 64))

    @torch.no_grad()
    def hip(self, images_u8):
        self.check_hip_widths()
        if (not torch.is_tensor(images_u8) or images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3
                or not images_u8.is_cuda or images_u8.numel() == 0):
            raise RuntimeError("RRDBNet.hip: expected a non-empty uint8 device tensor [B, H, W, 3]")
        B, H, W, _ = images_u8.shape
        r = self.unshuffle
        if H % r or W % r:
            raise ValueError(f"image sides must be multiples of {r} for the x{self.scale} network, got {W} x {H}")
        images_u8 = images_u8.contiguous()
        per = self.hip_batch_slice(H, W)
        outs = [self._hip_slice(images_u8[i:i + per]) for i in range(0, B, per)]
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    def _hip_slice(self, img):
        dev = img.device
        w = self._hip_weights(dev)
        conv = ops.dense_conv3x3
        cpad = self.hip_cpad
        f0 = ops.u8_unshuffle_f16(img, self.unshuffle, cpad)
        b, h, wd, _ = f0.shape
        # `first` takes conv_first's output, serves the first RRDB as its dense-block buffer and keeps channels [0, 64) for conv_body's residual:
        # nothing writes them again, since the first RRDB's result goes to a rotating buffer and `first` never joins the rotation
        first, *rot = [torch.empty((b, h, wd, 192), dtype=torch.float16, device=dev) for _ in range(4)]
        bufs = [first] + rot
        X, Y, Z = 0, 1, 2
        conv(f0, cpad, *w["conv_first"], first, 0, 64)
        for i in range(len(self.body)):
            src = X
            for j, dst in ((1, Y), (2, Z), (3, Y)):
                p = f"body.{i}.rdb{j}."
                for k in range(1, 5):
                    c = 64 + 32 * (k - 1)
                    conv(bufs[src], c, *w[p + f"conv{k}"], bufs[src], c, 32, slope=SLOPE)
                if j < 3:
                    conv(bufs[src], 192, *w[p + "conv5"], bufs[dst], 0, 64, r1=bufs[src], alpha=RES_SCALE)
                else:
                    conv(bufs[src], 192, *w[p + "conv5"], bufs[dst], 0, 64, r1=bufs[src], alpha=RES_SCALE, r2=bufs[X], beta=RES_SCALE)
                src = dst
            X = Y
            Y, Z = [k for k in (1, 2, 3) if k != X]
        Y = 1 if X != 1 else 2
        conv(bufs[X], 64, *w["conv_body"], bufs[Y], 0, 64, r1=first, alpha=1.0)
        u1 = torch.empty((b, 2 * h, 2 * wd, 64), dtype=torch.float16, device=dev)
        conv(bufs[Y], 64, *w["conv_up1"], u1, 0, 64, slope=SLOPE, upsample=True)
        del bufs, first, rot, f0
        u2 = torch.empty((b, 4 * h, 4 * wd, 64), dtype=torch.float16, device=dev)
        conv(u1, 64, *w["conv_up2"], u2, 0, 64, slope=SLOPE, upsample=True)
        del u1
        u3 = torch.empty_like(u2)
        conv(u2, 64, *w["conv_hr"], u3, 0, 64, slope=SLOPE)
        del u2
        return ops.dense_conv3x3_u8(u3, 64, *w["conv_last"], 3)


def expected_keys(scale, num_block):
    """{parameter name: shape} of the published RRDBNet layout (width 64, growth 32)."""
    keys = {}

    def add(name, cout, cin):
        keys[name + ".weight"], keys[name + ".bias"] = (cout, cin, 3, 3), (cout,)

    add("conv_first", 64, 3 * _UNSHUFFLE[scale] ** 2)
    for i in range(num_block):
        for j in (1, 2, 3):
            for k in range(1, 5):
                add(f"body.{i}.rdb{j}.conv{k}", 32, 64 + 32 * (k - 1))
            add(f"body.{i}.rdb{j}.conv5", 64, 192)
    for name in ("conv_body", "conv_up1", "conv_up2", "conv_hr"):
        add(name, 64, 64)
    add("conv_last", 3, 64)
    return keys


def load_esrgan(path_or_state_dict):
    """A Real-ESRGAN RRDBNet from a local ``.pth`` file or a state dict (``params_ema`` / ``params`` wrappers are unwrapped).  The scale comes
    from ``conv_first.weight.shape[1]`` (3 -> x4, 12 -> x2, 48 -> x1) and the block count from the keys.  Strict: missing, unexpected or
    mis-shaped keys raise ValueError naming them; widths other than 64 / 32 are refused.  Nothing is downloaded."""
    sd = path_or_state_dict
    if not isinstance(sd, dict):
        sd = torch.load(str(sd), map_location="cpu", weights_only=True)
    for wrap in ("params_ema", "params"):
        if wrap in sd and isinstance(sd[wrap], dict):
            sd = sd[wrap]
            break
    cf = sd.get("conv_first.weight")
    if not torch.is_tensor(cf) or cf.dim() != 4:
        raise ValueError("not an RRDBNet state dict: missing key conv_first.weight")
    if cf.shape[1] not in _SCALE_OF_IN_CH:
        raise ValueError(f"conv_first.weight takes {cf.shape[1]} channels: expected 3 (x4), 12 (x2) or 48 (x1)")
    scale = _SCALE_OF_IN_CH[cf.shape[1]]
    grow = sd.get("body.0.rdb1.conv1.weight")
    if cf.shape[0] != 64 or (torch.is_tensor(grow) and grow.shape[0] != 32):
        raise ValueError(f"only RRDBNet of width 64 with growth 32 is built, got conv_first.weight {tuple(cf.shape)}"
                         + (f" and body.0.rdb1.conv1.weight {tuple(grow.shape)}" if torch.is_tensor(grow) else ""))
    blocks = [int(m.group(1)) for m in (re.match(r"body\.(\d+)\.", k) for k in sd) if m]
    num_block = max(blocks) + 1 if blocks else 0
    want = expected_keys(scale, num_block)
    missing = sorted(k for k in want if k not in sd)
    unexpected = sorted(k for k in sd if k not in want)
    bad = sorted(f"{k} {tuple(sd[k].shape)} (expected {want[k]})" for k in want if k in sd and tuple(sd[k].shape) != want[k])
    if num_block == 0:
        missing = missing or ["body.0.rdb1.conv1.weight"]
    if missing or unexpected or bad:
        parts = [f"{n}: {', '.join(v[:8])}{' ...' if len(v) > 8 else ''}" for n, v in (("missing keys", missing), ("unexpected keys", unexpected),
                                                                                      ("mis-shaped keys", bad)) if v]
        raise ValueError(f"the state dict does not match RRDBNet x{scale} with {num_block} blocks -- " + "; ".join(parts))
    net = RRDBNet(scale=scale, num_block=num_block)
    net.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return net.eval()


class Upscaler:
    """The public object: ``upscaler(images)`` takes a uint8 tensor ``[B, H, W, 3]``, a PIL image or a list of equal-sized PIL images and
    returns the same kind, ``scale`` times the size.  Sides must be multiples of the network's unshuffle factor and at most 1024 pixels: both
    are a ValueError before any GPU work."""

    def __init__(self, net, device="cuda"):
        if not isinstance(net, RRDBNet):
            raise ValueError(f"Upscaler takes an RRDBNet (see load_esrgan), got {type(net).__name__}")
        net.check_hip_widths()
        self.net = net.eval()
        self.device = device
        self.scale = net.scale
        self.max_input_side = MAX_INPUT_SIDE

    def check_size(self, H, W):
        r = self.net.unshuffle
        if H < r or W < r or H % r or W % r:
            raise ValueError(f"the x{self.scale} upscaler takes image sides that are positive multiples of {r}, got {W} x {H}")
        if max(H, W) > self.max_input_side:
            raise ValueError(f"the upscaler's input may be at most {self.max_input_side} pixels on a side, got {W} x {H} (tiled upscaling is "
                             "not built)")

    def upscale_u8(self, images_u8):
        """uint8 [B, H, W, 3] on any device -> uint8 [B, sH, sW, 3] on ``self.device`` (batches are sliced inside RRDBNet.hip)."""
        if not torch.is_tensor(images_u8) or images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3 or images_u8.shape[0] < 1:
            raise ValueError("the upscaler takes a uint8 tensor [B, H, W, 3] with B >= 1")
        self.check_size(images_u8.shape[1], images_u8.shape[2])
        if next(self.net.parameters()).device.type != torch.device(self.device).type:
            self.net.to(self.device)                 # once: moving the network drops its prepared device weights
        return self.net.hip(images_u8.to(self.device).contiguous())

    def __call__(self, images):
        from PIL import Image
        import numpy as np
        if torch.is_tensor(images):
            return self.upscale_u8(images).to(images.device)
        single = isinstance(images, Image.Image)
        ims = [images] if single else list(images)
        if not ims or not all(isinstance(im, Image.Image) for im in ims):
            raise ValueError("the upscaler takes a uint8 tensor [B, H, W, 3], a PIL image or a non-empty list of PIL images")
        if any(im.size != ims[0].size for im in ims):
            raise ValueError(f"the images of a list must have one size, got {sorted({im.size for im in ims})}")
        self.check_size(ims[0].size[1], ims[0].size[0])
        arr = np.stack([np.asarray(im.convert("RGB"), dtype=np.uint8) for im in ims])
        out = self.upscale_u8(torch.from_numpy(arr)).cpu().numpy()
        pil = [Image.fromarray(o) for o in out]
        return pil[0] if single else pil
