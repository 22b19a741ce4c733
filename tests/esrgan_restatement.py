"""Helper of the Real-ESRGAN tests (no tests in here): an independent plain-torch walk of RRDBNet over a STATE DICT, built from F.conv2d,
F.pixel_unshuffle and F.interpolate(mode="nearest") only, restated from xinntao's basicsr/archs/rrdbnet_arch.py (restated, not pinned: no copy
of the reference is available offline).  It shares no code with adaface_dev_amd/adaface/esrgan.py.  ``rrdbnet_walk(..., store=f)`` applies ``f``
to every tensor the device path stores (fp16 rounding for walk B of tests/test_hip_esrgan.py); the default stores nothing differently."""
import math

import torch
import torch.nn.functional as F

UNSHUFFLE = {4: 1, 2: 2, 1: 4}


def conv_names(num_block):
    names = ["conv_first"]
    for i in range(num_block):
        for j in (1, 2, 3):
            names += [f"body.{i}.rdb{j}.conv{k}" for k in range(1, 6)]
    return names + ["conv_body", "conv_up1", "conv_up2", "conv_hr", "conv_last"]


def conv_shape(name, scale):
    """(cout, cin) of a convolution of the published layout."""
    if name == "conv_first":
        return 64, 3 * UNSHUFFLE[scale] ** 2
    if name == "conv_last":
        return 3, 64
    if name.startswith("body."):
        k = int(name[-1])
        return (64, 192) if k == 5 else (32, 64 + 32 * (k - 1))
    return 64, 64


def make_state_dict(scale, num_block, seed, gain=0.1):
    """Normal weights times gain / sqrt(9 cin), biases around 0 (std 0.01); conv_last: bias 0.5.

    gain = 0.1 (the default): conv_last's weights are normal times 6 / sqrt(9 cin), which spreads its outputs over about [-0.1, 1.1] for inputs
    of standard deviation 0.05 (the stand-alone uint8 kernel case).  Through a WHOLE network these weights attenuate the image by 0.1 per
    convolution: at conv_hr it is some 1000 times below conv_hr's own bias, the output is a per-channel constant away from the borders, and no
    test on it can see the unshuffle, conv_first, the body or the upsampling convolutions.

    The network-level tests therefore use gain = sqrt(2) (He's factor, which keeps the activations' magnitude through the LeakyReLU chain): the
    image and the body then dominate every later tensor.  There conv_last's weights are scaled from the network itself -- one fp64 walk of a
    fixed random 8 x 8 image -- so that the network's output on it has mean 0.5 and standard deviation 0.3: spread over about
    [-0.1, 1.1], with both clamps exercised."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name in conv_names(num_block):
        cout, cin = conv_shape(name, scale)
        if name == "conv_last":
            sd[name + ".weight"] = torch.randn(cout, cin, 3, 3, generator=g) * (6.0 / math.sqrt(9 * cin))
            sd[name + ".bias"] = torch.full((cout,), 0.5)
        else:
            sd[name + ".weight"] = torch.randn(cout, cin, 3, 3, generator=g) * (gain / math.sqrt(9 * cin))
            sd[name + ".bias"] = torch.randn(cout, generator=g) * 0.01
    if gain != 0.1:
        r = UNSHUFFLE[scale]
        x = torch.rand(1, 3, 8 * r, 8 * r, generator=g, dtype=torch.float64)
        out = rrdbnet_walk(sd, x, scale, num_block)
        k = 0.3 / float(out.std())
        sd["conv_last.weight"] = sd["conv_last.weight"] * k
        sd["conv_last.bias"] = torch.full((3,), 0.5 - k * (float(out.mean()) - 0.5))
    return sd


HE_GAIN = math.sqrt(2.0)
# (scale, num_block, B, H, W) of the network-level tests: 24 x 20 leaves partial patches on both axes of the body and of every tail stage;
# six blocks rotate the buffers over more than two RRDBs
NETWORK_CASES = [(4, 2, 2, 24, 20), (2, 2, 1, 24, 20), (4, 6, 1, 16, 16)]
_CASES = {}


def quantise(t):
    """[B, 3, H, W] in about [0, 1] -> levels [B, H, W, 3]: rint(255 clamp(t)), ties to even."""
    return torch.round(255 * t.clamp(0, 1)).permute(0, 2, 3, 1)


def network_case(scale, num_block, B, H, W, gain=HE_GAIN):
    """One network-level case, computed once and shared by the tests that use it: dict(sd, img uint8 [B, H, W, 3], x fp64 NCHW, a = walk A in
    fp64, want = quantise(a), e16 = max |255 B - 255 A| with walk B = fp32 convolutions and every stored tensor rounded to fp16)."""
    key = (scale, num_block, B, H, W, gain)
    if key not in _CASES:
        seed = 40 + scale + num_block
        sd = make_state_dict(scale, num_block, seed, gain)
        img = torch.randint(0, 256, (B, H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
        x = img.permute(0, 3, 1, 2).double() / 255
        a = rrdbnet_walk(sd, x, scale, num_block)
        b = rrdbnet_walk(sd, x.float(), scale, num_block, store=lambda t: t.half().to(t.dtype))
        _CASES[key] = dict(sd=sd, img=img, x=x, a=a, want=quantise(a), e16=float((255 * b.double() - 255 * a).abs().max()))
    return _CASES[key]


def rrdbnet_walk(sd, x, scale, num_block, store=lambda t: t, mutate=None):
    """x [B, 3, H, W] in [0, 1] -> [B, 3, sH, sW], in x's dtype.  ``store`` is applied wherever the device path writes a tensor to memory: the
    unshuffled input, every convolution's output after its fused activation / residuals.  ``mutate`` builds a deliberately WRONG network for
    the tests' sensitivity checks: "no_body" (conv_body sees conv_first's output), "stale_r2" (an RRDB's outer residual is the previous RRDB's
    input, what a wrong buffer rotation reads), "no_lrelu" (no activation inside the dense blocks)."""
    dt = x.dtype

    def conv(name, t):
        return F.conv2d(t, store(sd[name + ".weight"].to(dt)), sd[name + ".bias"].to(dt), padding=1)

    def lrelu(t):
        return torch.where(t >= 0, t, 0.2 * t)

    r = UNSHUFFLE[scale]
    f = store(F.pixel_unshuffle(x, r) if r > 1 else x)
    first = store(conv("conv_first", f))
    f = first
    prev_in = first
    for i in range(num_block if mutate != "no_body" else 0):
        rrdb_in = f
        for j in (1, 2, 3):
            p = f"body.{i}.rdb{j}."
            feats = [f]
            for k in range(1, 5):
                y = conv(p + f"conv{k}", torch.cat(feats, 1))
                feats.append(store(y if mutate == "no_lrelu" else lrelu(y)))
            x5 = conv(p + "conv5", torch.cat(feats, 1))
            if j < 3:
                f = store(0.2 * x5 + f)
            else:
                f = store(0.2 * (0.2 * x5 + f) + (prev_in if mutate == "stale_r2" else rrdb_in))
        prev_in = rrdb_in
    f = store(conv("conv_body", f) + first)
    f = store(lrelu(conv("conv_up1", F.interpolate(f, scale_factor=2, mode="nearest"))))
    f = store(lrelu(conv("conv_up2", F.interpolate(f, scale_factor=2, mode="nearest"))))
    f = store(lrelu(conv("conv_hr", f)))
    return conv("conv_last", f)
