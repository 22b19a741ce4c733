"""Helper of the GFPGAN tests (no tests in here): an independent functional walk of GFPGANv1Clean over a STATE DICT, built from F.conv2d (grouped,
for the modulated convolutions), F.linear and F.interpolate only, restated from TencentARC's gfpgan/archs/gfpganv1_clean_arch.py and
stylegan2_clean_arch.py (restated, not pinned: no copy of the reference is available offline).  It shares no code with
adaface_dev_amd/adaface/gfpgan.py.  ``gfpgan_walk(..., store=f)`` applies ``f`` to every tensor the device path stores (fp16 rounding for walk B
of tests/test_hip_gfpgan.py); the default stores nothing differently.  ``mutate`` builds deliberately WRONG networks for the sensitivity checks.

cfg = dict(out_size, num_style_feat, channel_multiplier, narrow)."""
import math

import torch
import torch.nn.functional as F

CFG32 = dict(out_size=32, num_style_feat=64, channel_multiplier=2, narrow=0.125)      # widths 32 (U-Net) / 64 (decoder)
CFG64 = dict(out_size=64, num_style_feat=64, channel_multiplier=2, narrow=0.25)       # widths 64 / 128
MUTATIONS = ("no_noise", "no_sft", "no_demod", "no_sqrt2", "no_skips", "nearest", "swap_sft")
LEVELS = 127.5


def widths(cfg, half):
    n = cfg["narrow"] * (0.5 if half else 1.0)
    cm = cfg["channel_multiplier"]
    t = {r: int(512 * n) for r in (4, 8, 16, 32)}
    t.update({64: int(256 * cm * n), 128: int(128 * cm * n), 256: int(64 * cm * n), 512: int(32 * cm * n)})
    return t


def key_shapes(cfg):
    """{state-dict key: shape}, written down here on its own (the tests compare it with the package's expected_keys)."""
    S, nsf = cfg["out_size"], cfg["num_style_feat"]
    L = int(math.log2(S))
    U, D = widths(cfg, True), widths(cfg, False)
    k = {"conv_body_first.weight": (U[S], 3, 1, 1), "conv_body_first.bias": (U[S],)}

    def res(p, ci, co):
        k.update({p + "conv1.weight": (ci, ci, 3, 3), p + "conv1.bias": (ci,), p + "conv2.weight": (co, ci, 3, 3), p + "conv2.bias": (co,),
                  p + "skip.weight": (co, ci, 1, 1)})

    def mod(p, co, ci, ks):
        k.update({p + "modulated_conv.weight": (1, co, ci, ks, ks), p + "modulated_conv.modulation.weight": (ci, nsf),
                  p + "modulated_conv.modulation.bias": (ci,)})

    ci = U[S]
    for j in range(L - 2):
        co = U[S >> (j + 1)]
        res(f"conv_body_down.{j}.", ci, co)
        ci = co
    k.update({"final_conv.weight": (U[4], ci, 3, 3), "final_conv.bias": (U[4],), "final_linear.weight": ((2 * L - 2) * nsf, 16 * U[4]),
              "final_linear.bias": ((2 * L - 2) * nsf,)})
    ci = U[4]
    for j in range(L - 2):
        c = U[8 << j]
        res(f"conv_body_up.{j}.", ci, c)
        k.update({f"toRGB.{j}.weight": (3, c, 1, 1), f"toRGB.{j}.bias": (3,)})
        for n in ("condition_scale", "condition_shift"):
            for q in (0, 2):
                k.update({f"{n}.{j}.{q}.weight": (c, c, 3, 3), f"{n}.{j}.{q}.bias": (c,)})
        ci = c
    d = "stylegan_decoder."
    for i in range(8):
        k.update({f"{d}style_mlp.{2 * i + 1}.weight": (nsf, nsf), f"{d}style_mlp.{2 * i + 1}.bias": (nsf,)})
    k[d + "constant_input.weight"] = (1, D[4], 4, 4)

    def style_conv(p, ci, co):
        mod(p, co, ci, 3)
        k.update({p + "weight": (1,), p + "bias": (1, co, 1, 1)})

    def to_rgb(p, ci):
        mod(p, 3, ci, 1)
        k[p + "bias"] = (1, 3, 1, 1)

    style_conv(d + "style_conv1.", D[4], D[4])
    to_rgb(d + "to_rgb1.", D[4])
    ci = D[4]
    for j in range(L - 2):
        c = D[8 << j]
        style_conv(f"{d}style_convs.{2 * j}.", ci, c)
        style_conv(f"{d}style_convs.{2 * j + 1}.", c, c)
        to_rgb(f"{d}to_rgbs.{j}.", c)
        ci = c
    for l in range(2 * (L - 2) + 1):
        r = 2 ** ((l + 5) // 2)
        k[f"{d}noises.noise{l}"] = (1, 1, r, r)
    return k


def make_state_dict(cfg, seed):
    """Weights under which every branch matters (torch's default initialisation gives |output| ~ 0.2 and tests that see nothing): He-scaled plain
    convolutions with biases of 0.1, ResBlock outputs kept at unit scale, noise weights in [0.1, 0.3], StyleConv biases of 0.2, modulation
    biases 1 + 0.5 randn with weights that add another 0.5 randn, and the condition branches' last convolutions scaled FROM THE NETWORK ITSELF
    -- one fp64 walk of a fixed random input -- so that scale = 1 +- 0.5 and shift = +- 0.5.  The output is of order 1."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    sd = {}
    for name, shape in key_shapes(cfg).items():
        if name.endswith("modulated_conv.weight"):
            fan = shape[2] * shape[3] * shape[4]
            sd[name] = rn(*shape) * ((0.6 if shape[1] == 3 else 1.0) / math.sqrt(fan))
        elif name.endswith("modulation.weight"):
            sd[name] = rn(*shape) * (0.5 / math.sqrt(shape[1]))
        elif name.endswith("modulation.bias"):
            sd[name] = 1.0 + 0.5 * rn(*shape)
        elif "noises." in name or name.endswith("constant_input.weight"):
            sd[name] = rn(*shape)
        elif name.startswith("stylegan_decoder.style_mlp") or name.startswith("toRGB"):
            sd[name] = rn(*shape) * 0.05                             # loaded, never run
        elif name.startswith("stylegan_decoder.") and name.endswith(".weight"):         # a StyleConv's noise weight
            sd[name] = 0.1 + 0.2 * torch.rand(*shape, generator=g)
        elif name.startswith("stylegan_decoder.") and name.endswith(".bias"):
            sd[name] = rn(*shape) * (0.1 if shape[1] == 3 else 0.2)
        elif name.endswith(".bias"):
            sd[name] = rn(*shape) * 0.1
        elif name == "final_linear.weight":
            sd[name] = rn(*shape) / math.sqrt(shape[1])
        else:                                                       # a plain convolution
            fan = shape[1] * shape[2] * shape[3]
            gain = math.sqrt(2.0)
            if ".conv2." in name or ".skip." in name:
                gain = 1.0 if ".conv2." in name else math.sqrt(0.5)  # out + skip stays at unit scale
            sd[name] = rn(*shape) * (gain / math.sqrt(fan))
    x = torch.rand(2, 3, cfg["out_size"], cfg["out_size"], generator=g, dtype=torch.float64) * 2 - 1
    probe = {}
    gfpgan_walk(sd, x, cfg, probe=probe)
    for j in range(int(math.log2(cfg["out_size"])) - 2):
        for n, centre in (("condition_scale", 1.0), ("condition_shift", 0.0)):
            p = f"{n}.{j}.2."
            raw = probe[f"{n}.{j}"] - sd[p + "bias"].double().view(1, -1, 1, 1)
            sd[p + "weight"] = sd[p + "weight"] * (0.5 / float(raw.std()))
            sd[p + "bias"] = centre + 0.05 * rn(*sd[p + "bias"].shape)
    return sd


def gfpgan_walk(sd, x, cfg, store=lambda t: t, mutate=None, probe=None):
    """x [B, 3, S, S] in [-1, 1] -> [B, 3, S, S], in x's dtype.  ``store`` is applied wherever the device path writes a tensor to memory: the
    fp16 weights of the plain convolutions and linears, every convolution's output, every activation pass, every resampled map, the latents,
    the per-sample modulated weights (gain included) and every epilogue output.  ``probe`` (a dict) receives the condition maps."""
    assert mutate is None or mutate in MUTATIONS
    dt = x.dtype
    S = cfg["out_size"]
    n = int(math.log2(S)) - 2
    P = lambda k: sd[k].to(dt)

    def lrelu(t):
        return torch.where(t >= 0, t, 0.2 * t)

    def conv(name, t):
        w = P(name + ".weight")
        b = P(name + ".bias") if name + ".bias" in sd else None
        return store(F.conv2d(t, store(w), b, padding=w.shape[-1] // 2))

    def act(t):
        return store(lrelu(t))

    def up(t):
        if mutate == "nearest":
            return F.interpolate(t, scale_factor=2, mode="nearest")
        return F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)

    def resblock(p, t, mode):
        rs = (lambda v: store(F.interpolate(v, scale_factor=0.5, mode="bilinear", align_corners=False))) if mode == "down" else (lambda v: store(up(v)))
        out = act(conv(p + "conv1", t))
        out = act(conv(p + "conv2", rs(out)))
        w = store(P(p + "skip.weight"))
        return store(F.conv2d(rs(t), w) + out)

    feat = act(conv("conv_body_first", store(x)))
    skips = []
    for j in range(n):
        feat = resblock(f"conv_body_down.{j}.", feat, "down")
        skips.insert(0, feat)
    feat = act(conv("final_conv", feat))
    B = x.shape[0]
    nsf = cfg["num_style_feat"]
    latent = store(F.linear(feat.reshape(B, -1), store(P("final_linear.weight")), P("final_linear.bias"))).view(B, -1, nsf)
    conds = []
    for j in range(n):
        if mutate != "no_skips":
            feat = store(feat + skips[j])
        feat = resblock(f"conv_body_up.{j}.", feat, "up")
        pair = []
        for name in ("condition_scale", "condition_shift"):
            c = conv(f"{name}.{j}.2", act(conv(f"{name}.{j}.0", feat)))
            if probe is not None:
                probe[f"{name}.{j}"] = c
            pair.append(c)
        conds.append(pair[::-1] if mutate == "swap_sft" else pair)

    def modconv(p, t, style, demod, gain, upsample):
        w = P(p + "modulated_conv.weight")                           # [1, co, ci, k, k]
        s = F.linear(style, store(P(p + "modulated_conv.modulation.weight")), P(p + "modulated_conv.modulation.bias"))
        w = w * s.view(B, 1, -1, 1, 1)
        if demod and mutate != "no_demod":
            w = w * torch.rsqrt((w * w).sum(dim=(2, 3, 4), keepdim=True) + 1e-8)
        w = store(w * gain)
        co, ci, k = w.shape[1], w.shape[2], w.shape[3]
        if upsample:
            t = store(up(t))
        h, wd = t.shape[2:]
        y = F.conv2d(t.reshape(1, B * ci, h, wd), w.reshape(B * co, ci, k, k), padding=k // 2, groups=B)
        return y.view(B, co, h, wd)

    d = "stylegan_decoder."

    def style_conv(p, t, style, l, upsample=False, sft=None):
        y = store(modconv(p, t, style, True, 1.0 if mutate == "no_sqrt2" else math.sqrt(2.0), upsample))
        nw = 0.0 if mutate == "no_noise" else P(p + "weight")
        v = lrelu(y + nw * P(f"{d}noises.noise{l}") + P(p + "bias"))
        if sft is not None and mutate != "no_sft":
            half = v.shape[1] // 2
            v = torch.cat([v[:, :half], v[:, half:] * sft[0] + sft[1]], dim=1)
        return store(v)

    def to_rgb(p, t, style, skip):
        rgb = store(modconv(p, t, style, False, 1.0, False) + P(p + "bias"))
        return rgb if skip is None else store(up(skip) + rgb)

    const = store(P(d + "constant_input.weight"))
    out = style_conv(d + "style_conv1.", const.expand(B, -1, -1, -1), latent[:, 0], 0)
    skip = to_rgb(d + "to_rgb1.", out, latent[:, 1], None)
    i = 1
    for j in range(n):
        out = style_conv(f"{d}style_convs.{2 * j}.", out, latent[:, i], 2 * j + 1, upsample=True, sft=conds[j])
        out = style_conv(f"{d}style_convs.{2 * j + 1}.", out, latent[:, i + 1], 2 * j + 2)
        skip = to_rgb(f"{d}to_rgbs.{j}.", out, latent[:, i + 2], skip)
        i += 2
    return skip


_CASES = {}


def network_case(name):
    """One network-level case ("32" or "64"), computed once and shared: dict(cfg, sd, x fp64 [2, 3, S, S] of fp16-representable values in
    [-1, 1], a = walk A in fp64, e16 = 127.5 max |B - A| with walk B in fp32 and every stored tensor rounded to fp16)."""
    if name not in _CASES:
        cfg = {"32": CFG32, "64": CFG64}[name]
        seed = 70 + cfg["out_size"]
        sd = make_state_dict(cfg, seed)
        g = torch.Generator().manual_seed(seed + 1)
        x = (torch.rand(2, 3, cfg["out_size"], cfg["out_size"], generator=g) * 2 - 1).half().double()
        a = gfpgan_walk(sd, x, cfg)
        b = gfpgan_walk(sd, x.float(), cfg, store=lambda t: t.half().to(t.dtype))
        _CASES[name] = dict(cfg=cfg, sd=sd, x=x, a=a, e16=LEVELS * float((b.double() - a).abs().max()))
    return _CASES[name]
