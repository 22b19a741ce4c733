"""The kernels of the GFPGAN face restorer on a real MI355X (`pytest -m gpu`), through the C entry points (INTEGRATION.md "Face restoration
(GFPGAN)"): af_modulate_weights, af_style_epilogue, af_bilinear_up2, af_face_align_crop_any and af_face_paste_affine_u8, each against its
formula in include/adaface_hip.h evaluated in fp64 on the CPU from the same inputs; nothing in a reference comes from a kernel.

Bound for an fp16 output: 2^-10 |ref| + 2^-24 + 4 e32 per element.  The first term is one fp16 rounding (2^-11 relative) with room, the second
the spacing of fp16's subnormals, and e32 is the largest error of an fp32 numpy evaluation of the same formula against fp64 (the kernels work
in fp32 too, in another order where there is a sum).  Outputs start filled with a sentinel, so an element a kernel does not write shows."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_hip_face_id import INV_SMALL, _crop_reference

pytestmark = pytest.mark.gpu

SENTINEL = 0x7ABC          # an fp16 bit pattern (finite, 54144.0) no result takes
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _sentinel(shape, dev):
    return torch.zeros(shape, dtype=torch.int16, device=dev).fill_(SENTINEL).view(torch.float16)


def _check_f16(got, ref64, ref32, what):
    e32 = float(np.abs(ref32.astype(np.float64) - ref64).max())
    bound = 2.0 ** -10 * np.abs(ref64) + U + 4 * e32
    err = np.abs(got.astype(np.float64) - ref64)
    print(f"{what}: max |kernel - fp64| = {err.max():.3e} (max |ref| {np.abs(ref64).max():.3e}, e32 {e32:.2e}), worst err / bound = {(err / bound).max():.3f}")
    assert np.isfinite(got).all() and (err <= bound).all(), what


def _p(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------------------------- af_modulate_weights
def modulate_formula(w, wsq, s, gain, demod, dt):
    """[B, cout, taps * cin] in dtype dt: gain * d[b,o] * w[o,t,i] * s[b,i], d = 1 / sqrt(sum_i s^2 wsq + 1e-8)."""
    w, s = w.astype(dt), s.astype(dt)
    d = np.ones((s.shape[0], w.shape[0]), dtype=dt)
    if demod:
        d = dt(1) / np.sqrt(((s * s)[:, None, :] * wsq.astype(dt)[None]).sum(axis=2) + dt(1e-8))
    out = (dt(gain) * d)[:, :, None, None] * w[None] * s[:, None, None, :]
    return out.reshape(s.shape[0], w.shape[0], -1)


def _modulate(dev, B, cout, cin, taps, demod, gain, style_scale, seed):
    from adaface_dev_amd import _lib
    g = np.random.default_rng(seed)
    w = (g.standard_normal((cout, taps, cin)) / np.sqrt(taps * cin)).astype(np.float32)
    wsq = (w * w).sum(axis=1).astype(np.float32)
    s = ((1.0 + 0.5 * g.standard_normal((B, cin))) * style_scale).astype(np.float32)
    K, npad, kpad = taps * cin, (cout + 127) // 128 * 128, (taps * cin + 63) // 64 * 64
    out = torch.zeros((B, npad, kpad), dtype=torch.float16, device=dev)          # the padding is the caller's zeros
    out[:, :cout, :K] = _sentinel((B, cout, K), dev)
    tw, tq, ts = (torch.from_numpy(a).to(dev) for a in (w, wsq, s))
    rc = _lib.lib().af_modulate_weights(_p(tw), _p(tq) if demod else None, _p(ts), _p(out), B, cout, cin, taps, npad, kpad, int(demod), gain, None)
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().af_last_error()
    return w, wsq, s, out.cpu(), (tw, tq, ts)


@pytest.mark.parametrize("cout,cin,taps,demod,style_scale", [(24, 40, 9, True, 1.0), (3, 64, 1, False, 1.0), (64, 64, 9, True, 1000.0)],
                         ids=["24x40x9", "rgb3x64x1-nodemod", "64x64x9-styles-x1000"])
def test_modulate_weights(dev, cout, cin, taps, demod, style_scale):
    """B = 2 with distinct styles.  (24, 40, 9): K = 360 -> kpad 384, npad 128, so there are rows and columns of padding behind the block, and
    the reduction over 40 channels fills less than one wave.  (3, 64, 1): the RGB form, no demodulation.  Styles x 1000: d absorbs
    them, the weights stay finite and equal to the unscaled ones within the bound.  The padding stays zero; slice b does not depend on the
    other slice."""
    from adaface_dev_amd import _lib
    gain = 2.0 ** 0.5 if demod else 1.0
    w, wsq, s, out, (tw, tq, ts) = _modulate(dev, 2, cout, cin, taps, demod, gain, style_scale, seed=cout + cin)
    K = taps * cin
    got = out[:, :cout, :K].float().numpy()
    assert not (out[:, :cout, :K].view(torch.int16) == SENTINEL).any()
    _check_f16(got, modulate_formula(w, wsq, s, gain, demod, np.float64), modulate_formula(w, wsq, s, gain, demod, np.float32),
               f"modulate_weights ({cout}, {cin}, {taps}) demod {demod} styles x{style_scale:g}")
    pad = out.clone()
    pad[:, :cout, :K] = 0
    assert not pad.view(torch.int16).any()                                           # rows cout .. npad and columns K .. kpad: still zero bits
    assert float(np.abs(got[0] - got[1]).max()) > 0.01                               # two styles, two sets of weights
    if demod:
        norms = np.sqrt((got.astype(np.float64) ** 2).sum(axis=2))
        assert np.abs(norms - gain).max() < 2e-3                                     # unit-norm rows (times gain), whatever the styles' scale
    # slice 1 alone (as sample 0 of a batch of one) gives the same bits
    npad, kpad = out.shape[1:]
    alone = torch.zeros((1, npad, kpad), dtype=torch.float16, device=dev)
    rc = _lib.lib().af_modulate_weights(_p(tw), _p(tq) if demod else None, ts[1:].data_ptr(), _p(alone), 1, cout, cin, taps, npad, kpad, int(demod),
                                        gain, None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(alone.cpu()[0], out[1])


def test_modulate_weights_through_ops_feeds_the_convolution(dev):
    """ops.modulate_weights + one ops.conv3x3 per sample on a PackedWeight view of slice b == the grouped-convolution form of
    ModulatedConv2d in fp64 (cout 24 -> N = 24, cin 40, 5 x 7 pixels), within the fp16 rounding of weights and output."""
    from adaface_dev_amd import ops
    g = torch.Generator().manual_seed(5)
    B, cout, cin, H, W = 2, 24, 40, 5, 7
    w = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    s = 1.0 + 0.5 * torch.randn(B, cin, generator=g)
    x = torch.randn(B, H, W, cin, generator=g).half()
    wm = w.permute(0, 2, 3, 1).reshape(cout, 9, cin).contiguous()
    buf = torch.zeros((B, 128, 384), dtype=torch.float16, device=dev)
    wt = ops.modulate_weights(wm.to(dev), (wm * wm).sum(1).to(dev), s.to(dev), buf, gain=1.0)
    y = torch.empty((B, H, W, cout), dtype=torch.float16, device=dev)
    xd = x.to(dev)
    for b in range(B):
        ops.conv3x3(xd[b:b + 1], ops.PackedWeight(wt[b], None, cout, 9 * cin, 384, 9, cin), out=y[b:b + 1])
    torch.cuda.synchronize()
    wd = w.double()[None] * s.double()[:, None, :, None, None]
    wd = wd * torch.rsqrt((wd * wd).sum(dim=(2, 3, 4), keepdim=True) + 1e-8)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2).reshape(1, B * cin, H, W), wd.reshape(B * cout, cin, 3, 3), padding=1, groups=B)
    ref = ref.view(B, cout, H, W).permute(0, 2, 3, 1)
    err = float((y.cpu().double() - ref).abs().max())
    # each weight is rounded to fp16 once (2^-11 relative): sum_k |w_k| 2^-11 |x_k| <= 2^-11 sqrt(K) ||w||_2 max|x| with ||w||_2 = 1 (demodulated rows),
    # K = 360; the output's own rounding and the fp32 accumulation fit in 2^-10 max|ref|
    bound = 2.0 ** -11 * 360 ** 0.5 * float(x.float().abs().max()) + 2.0 ** -10 * float(ref.abs().max())
    print(f"modulated conv3x3 through ops: max |device - fp64| = {err:.3e}, bound {bound:.3e}, max |ref| {float(ref.abs().max()):.2f}")
    assert err <= bound


# ---------------------------------------------------------------------------------------------------------------- af_style_epilogue
def epilogue_formula(y, noise, bias, scale, shift, nw, dt):
    """y [B, HW, C] -> the header's formula in dtype dt."""
    v = y.astype(dt) + dt(nw) * noise.astype(dt)[None, :, None]
    v = v + bias.astype(dt)[None, None, :]
    v = np.where(v >= 0, v, dt(0.2) * v)
    if scale is not None:
        half = y.shape[2] // 2
        v = np.concatenate([v[..., :half], v[..., half:] * scale.astype(dt) + shift.astype(dt)], axis=2)
    return np.clip(v, dt(-65504.0), dt(65504.0))


def _epilogue(dev, y, noise, bias, scale, shift, nw):
    from adaface_dev_amd import _lib
    B, HW, C = y.shape
    ty = torch.from_numpy(y).to(dev)
    tn, tb = torch.from_numpy(noise).to(dev), torch.from_numpy(bias).to(dev)
    tsc, tsh = (None, None) if scale is None else (torch.from_numpy(scale).to(dev), torch.from_numpy(shift).to(dev))
    out = _sentinel((B, HW, C), dev)
    rc = _lib.lib().af_style_epilogue(_p(ty), _p(tn), _p(tb), _p(tsc), _p(tsh), _p(out), B, HW, C, nw, None)
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().af_last_error()
    assert not (out.view(torch.int16) == SENTINEL).any()
    return out.cpu().float().numpy()


@pytest.mark.parametrize("sft", [False, True], ids=["plain", "sft"])
@pytest.mark.parametrize("nw", [0.25, 0.0])
def test_style_epilogue(dev, sft, nw):
    """B = 2, 5 x 7 pixels, C = 48 (the SFT half starts at channel 24: a piece boundary that is no multiple of 16): with and without the SFT
    pointers, with a noise weight and with nw = 0."""
    g = np.random.default_rng(11)
    B, HW, C = 2, 35, 48
    y = g.standard_normal((B, HW, C)).astype(np.float16)
    noise, bias = g.standard_normal(HW).astype(np.float32), (0.2 * g.standard_normal(C)).astype(np.float32)
    scale = (1 + 0.5 * g.standard_normal((B, HW, C // 2))).astype(np.float16) if sft else None
    shift = (0.5 * g.standard_normal((B, HW, C // 2))).astype(np.float16) if sft else None
    got = _epilogue(dev, y, noise, bias, scale, shift, nw)
    ref = epilogue_formula(y, noise, bias, scale, shift, nw, np.float64)
    _check_f16(got, ref, epilogue_formula(y, noise, bias, scale, shift, nw, np.float32), f"style_epilogue sft={sft} nw={nw}")
    if sft:                                             # the lower half is untouched by the SFT, the upper half is not
        plain = epilogue_formula(y, noise, bias, None, None, nw, np.float64)
        assert np.abs(ref[..., :24] - plain[..., :24]).max() == 0 and np.abs(ref[..., 24:] - plain[..., 24:]).max() > 0.5
    if nw:
        assert np.abs(ref - epilogue_formula(y, noise, bias, scale, shift, 0.0, np.float64)).max() > 0.1


def test_style_epilogue_saturates_instead_of_overflowing(dev):
    """Inputs whose result leaves fp16's range come out as +-65504, not inf: by the bias (60000 + 10000), and by the SFT (x 8 after the
    LeakyReLU of -60000)."""
    B, HW, C = 1, 3, 16
    y = np.zeros((B, HW, C), dtype=np.float16)
    y[0, 0, :], y[0, 1, :], y[0, 2, :] = 60000.0, -60000.0, 1.0
    noise, bias = np.zeros(HW, dtype=np.float32), np.full(C, 10000.0, dtype=np.float32)
    scale, shift = np.full((B, HW, C // 2), 8.0, dtype=np.float16), np.zeros((B, HW, C // 2), dtype=np.float16)
    got = _epilogue(dev, y, noise, bias, scale, shift, 0.0)
    assert np.isfinite(got).all()
    assert (got[0, 0] == 65504.0).all()                                                   # 70000, and 560000 behind the SFT
    assert (got[0, 1, :8] == np.float16(0.2 * -50000.0)).all() and (got[0, 1, 8:] == -65504.0).all()   # -10000; x 8 = -80000 saturates
    assert (got[0, 2, :8] == np.float16(10001.0)).all() and (got[0, 2, 8:] == 65504.0).all()


# ---------------------------------------------------------------------------------------------------------------- af_bilinear_up2
def up2_formula(x, addend, dt):
    """x [B, H, W, C] -> [B, 2H, 2W, C], the header's formula in dtype dt."""
    def axis(n):
        o = np.arange(2 * n)
        k, odd = o // 2, (o & 1).astype(bool)
        return np.clip(np.where(odd, k, k - 1), 0, n - 1), np.clip(np.where(odd, k + 1, k), 0, n - 1), np.where(odd, 0.75, 0.25).astype(dt)

    x = x.astype(dt)
    y0, y1, wy0 = axis(x.shape[1])
    x0, x1, wx0 = axis(x.shape[2])
    wx0, wy0 = wx0[None, None, :, None], wy0[None, :, None, None]
    top = wx0 * x[:, y0][:, :, x0] + (dt(1) - wx0) * x[:, y0][:, :, x1]
    bot = wx0 * x[:, y1][:, :, x0] + (dt(1) - wx0) * x[:, y1][:, :, x1]
    v = wy0 * top + (dt(1) - wy0) * bot
    return v if addend is None else v + addend.astype(dt)


@pytest.mark.parametrize("add", [False, True], ids=["plain", "addend"])
@pytest.mark.parametrize("C", [8, 24])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (4, 4)])
def test_bilinear_up2(dev, H, W, C, add):
    """1 x 1 (every tap clamps onto the one pixel), 3 x 5 (odd, unequal sides), 4 x 4; C = 8 (one piece per pixel) and 24; B = 2.  The formula
    itself is pinned to F.interpolate(scale_factor=2, mode="bilinear", align_corners=False) in fp64."""
    from adaface_dev_amd import _lib
    g = np.random.default_rng(H * 10 + W + C)
    x = g.standard_normal((2, H, W, C)).astype(np.float16)
    a = g.standard_normal((2, 2 * H, 2 * W, C)).astype(np.float16) if add else None
    ref = up2_formula(x, a, np.float64)
    torch_ref = F.interpolate(torch.from_numpy(x).double().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    assert np.abs(up2_formula(x, None, np.float64) - torch_ref.numpy()).max() < 1e-12
    tx, ta = torch.from_numpy(x).to(dev), None if a is None else torch.from_numpy(a).to(dev)
    out = _sentinel((2, 2 * H, 2 * W, C), dev)
    rc = _lib.lib().af_bilinear_up2(_p(tx), _p(ta), _p(out), 2, H, W, C, None)
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().af_last_error()
    assert not (out.view(torch.int16) == SENTINEL).any()
    _check_f16(out.cpu().float().numpy(), ref, up2_formula(x, a, np.float32), f"bilinear_up2 {H}x{W} C={C} addend={add}")


# ---------------------------------------------------------------------------------------------------------------- af_face_align_crop_any
def test_face_align_crop_any_at_64(dev):
    """S = 64 through the new entry against the fp64 rule of tests/test_hip_face_id.py (same kernel, same bound 2^-10 for an image below
    512 pixels); the recogniser's entry still refuses 64."""
    from adaface_dev_amd import _lib, ops
    img = np.random.default_rng(41).integers(0, 256, size=(37, 53, 3), dtype=np.uint8)
    inv = (INV_SMALL * np.array([[[1.75, 1.75, 1.0]]], dtype=np.float32)).astype(np.float32)       # 112 -> 64 output pixels over the same region
    ref, n_in = _crop_reference(img, inv, 64)
    assert n_in[0].min() == 4 and (n_in[1] == 0).any() and (n_in[1] == 4).any()
    ti, tm = torch.from_numpy(img).to(dev), torch.from_numpy(inv).to(dev)
    out = _sentinel((3, 64, 64, 8), dev)
    rc = _lib.lib().af_face_align_crop_any(_p(ti), _p(tm), _p(out), 37, 53, 3, 64, None)
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().af_last_error()
    got = out.cpu().float().numpy()
    err = float(np.abs(got[..., :3] - ref).max())
    print(f"face_align_crop_any 64: max |kernel - fp64 rule| = {err:.3e}")
    assert err <= 2.0 ** -10 and (got[..., 3:] == 0).all()
    assert torch.equal(ops.face_align_crop_any(ti, tm, 64), out)
    assert _lib.lib().af_face_align_crop(_p(ti), _p(tm), _p(out), 37, 53, 3, 64, None) == _lib.AF_E_BADARG
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.face_align_crop_any(ti, tm, 60)


# ---------------------------------------------------------------------------------------------------------------- af_face_paste_affine_u8
def _similarity(scale, theta, tx, ty):
    c, s = scale * np.cos(theta), scale * np.sin(theta)
    return np.array([[c, -s, tx], [s, c, ty]], dtype=np.float32)


def paste_formula(photo, crops, mats, erode, feather):
    """The header's formula in fp64, coordinates from the same fp32 matrices -> (v64 [H, W, 3] before the final rounding, m [F, H, W])."""
    H, W, _ = photo.shape
    S = crops.shape[1]
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    cur = photo.astype(np.float64)
    ms = []
    for f, M in enumerate(mats.astype(np.float64)):
        u, v = M[0, 0] * xs + M[0, 1] * ys + M[0, 2], M[1, 0] * xs + M[1, 1] * ys + M[1, 2]
        m = np.minimum(np.minimum(u, v), np.minimum(S - 1 - u, S - 1 - v))
        ms.append(m)
        on = m > erode
        t = np.clip((m - erode) / feather, 0.0, 1.0) if feather > 0 else np.ones_like(m)
        alpha = np.where(on, t * t * (3 - 2 * t), 0.0)[..., None]
        x0, y0 = np.clip(np.floor(u), 0, S - 2).astype(np.int64), np.clip(np.floor(v), 0, S - 2).astype(np.int64)
        ax, ay = (u - x0)[..., None], (v - y0)[..., None]
        c = crops[f].astype(np.float64)[..., :3]
        bil = (1 - ay) * ((1 - ax) * c[y0, x0] + ax * c[y0, x0 + 1]) + ay * ((1 - ax) * c[y0 + 1, x0] + ax * c[y0 + 1, x0 + 1])
        g = 255.0 * np.clip(bil / 2 + 0.5, 0.0, 1.0)
        cur = alpha * g + (1 - alpha) * cur
    return cur, np.stack(ms) if ms else np.zeros((0, H, W))


def paste_delta(crops, mats, H, W, feather):
    """What fp32 may add to |out - v64| beyond the final rounding's 0.5, per face and summed over the faces (a later face passes an earlier
    one's error on with a factor 1 - alpha <= 1); and e_m, twice the largest fp32 error of an m (the margin around m = erode inside which
    fp32 and fp64 may disagree on whether a face touches a pixel).  With u = 2^-24:
    * a coordinate is two products and two sums of magnitude at most c = |m0| W + |m1| H + |m2|: e_c = 4 u c; S - 1 - u adds u S;
    * alpha has slope at most 1.5 / feather in m, and t, t t, 3 - 2 t and the product add at most 6 u: e_a = (1.5 / feather)(e_c + u S) + 6 u;
    * the bilinear colour moves by at most G / 2 per crop pixel and axis, G = the largest difference of neighbouring crop values, so the
      coordinates cost 255 G e_c, and its ~12 operations on values of at most 255 cost 12 * 255 u;
    * the blend alpha g + (1 - alpha) cur: 255 e_a from alpha's error and 4 more roundings of 255 u."""
    S = crops.shape[1]
    total, e_m = 0.0, 0.0
    for f, M in enumerate(np.abs(mats.astype(np.float64))):
        c = max(M[0, 0] * W + M[0, 1] * H + M[0, 2], M[1, 0] * W + M[1, 1] * H + M[1, 2])
        e_c = 4 * U * c
        e_a = (1.5 / feather) * (e_c + U * S) + 6 * U
        cf = crops[f].astype(np.float64)[..., :3]
        G = max(np.abs(np.diff(cf, axis=0)).max(), np.abs(np.diff(cf, axis=1)).max())
        total += 255 * G * e_c + 255 * e_a + 16 * 255 * U
        e_m = max(e_m, e_c + U * S)
    return total, 2 * e_m


def _paste(dev, photo, crops, mats, S, ld, erode, feather):
    from adaface_dev_amd import _lib
    H, W, _ = photo.shape
    nf = 0 if crops is None else crops.shape[0]
    tp = torch.from_numpy(photo).to(dev)
    tc = None if crops is None else torch.from_numpy(crops).to(dev)
    tm = None if mats is None else torch.from_numpy(mats).to(dev)
    out = torch.full((H, W, 3), 0x5A, dtype=torch.uint8, device=dev)
    rc = _lib.lib().af_face_paste_affine_u8(_p(tp), _p(tc), _p(tm), _p(out), H, W, nf, S, ld, erode, feather, None)
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().af_last_error()
    return out.cpu().numpy()


def test_face_paste_affine_u8(dev):
    """Photo 67 x 91, S = 64, ld = 8: two overlapping faces under rotated similarities, the second reaching outside the photo.
    |out - v64| <= 0.5 + delta (``paste_delta``); where every face's m is at or below erode (by more than the coordinate error) the photo's
    bytes, bit for bit; such pixels, blended pixels and pixels under both faces all exist."""
    g = np.random.default_rng(23)
    H, W, S = 67, 91, 64
    erode, feather = float(np.float32(3.2)), float(np.float32(6.4))                     # 0.05 S and 0.10 S, as the kernel receives them
    photo = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    crops = np.zeros((2, S, S, 8), dtype=np.float16)
    crops[..., :3] = g.uniform(-1.2, 1.2, (2, S, S, 3))                                 # values outside [-1, 1] too: the clamp works
    crops[..., 3:] = 7.0                                                                # never read
    mats = np.stack([_similarity(1.31, 0.21, -14.3, -9.6), _similarity(0.93, -0.33, -38.2, 11.7)])
    got = _paste(dev, photo, crops, mats, S, 8, erode, feather)
    v64, m = paste_formula(photo, crops, mats, erode, feather)
    delta, e_m = paste_delta(crops, mats, H, W, feather)
    err = np.abs(got.astype(np.float64) - v64).max()
    print(f"face_paste_affine_u8: max |out - v64| = {err:.6f}, bound 0.5 + {delta:.2e}")
    assert err <= 0.5 + delta
    untouched = (m <= erode - e_m).all(axis=0)
    blended = (m > erode + e_m).any(axis=0)
    both = (m > erode + feather).all(axis=0)
    assert untouched.any() and blended.any() and both.any() and (untouched | blended).mean() > 0.99
    assert np.array_equal(got[untouched], photo[untouched])
    assert (got[blended] != photo[blended]).any()
    # the second face's crop reaches outside the photo: its corner (0, 0) maps to a negative image coordinate
    inv = np.linalg.inv(np.vstack([mats[1].astype(np.float64), [0, 0, 1]]))
    corners = np.array([[0, 0, 1], [S - 1, 0, 1], [0, S - 1, 1], [S - 1, S - 1, 1]]) @ inv.T
    assert (corners[:, 0].min() < 0 or corners[:, 1].min() < 0 or corners[:, 0].max() > W - 1 or corners[:, 1].max() > H - 1)
    # the tensor-level wrapper gives the same bytes
    from adaface_dev_amd import ops
    tp = torch.from_numpy(photo).to(dev)
    same = ops.face_paste_affine_u8(tp, torch.from_numpy(crops).to(dev), torch.from_numpy(mats).to(dev), erode, feather)
    assert np.array_equal(same.cpu().numpy(), got)


def test_face_paste_affine_u8_without_faces_is_a_copy(dev):
    from adaface_dev_amd import ops
    photo = np.random.default_rng(3).integers(0, 256, (67, 91, 3), dtype=np.uint8)
    assert np.array_equal(_paste(dev, photo, None, None, 0, 0, 3.2, 6.4), photo)
    assert np.array_equal(ops.face_paste_affine_u8(torch.from_numpy(photo).to(dev), None, None, 3.2, 6.4).cpu().numpy(), photo)
