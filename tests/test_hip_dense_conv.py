"""af_dense_conv3x3 and af_u8_unshuffle_f16 on a real MI355X (`pytest -m gpu`), through the C entry points (INTEGRATION.md "Upscaling
(Real-ESRGAN)").  The reference is the header's formula in fp64 on the CPU from the same fp16-rounded inputs and weights; nothing in it comes
from the kernel.

Bound per case (fp16 output): 2^-10 max|ref| + 4 e32.  The first term is one fp16 rounding of the output (2^-11 relative) with room; e32 is
the largest error of an fp32 torch CPU evaluation of the whole formula against fp64 (the kernel accumulates in fp32 too, in another order).
On the CPU at cin = 192, 19 x 21: e32 ~ 1e-6, the fp16 rounding alone 9.7e-4 under a bound of 3.6e-3."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from esrgan_restatement import make_state_dict

pytestmark = pytest.mark.gpu

SENTINEL = 0x7ABC          # an fp16 bit pattern (finite, 54144.0) no result takes


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def make_case(B, H, W, cin, cout, seed, ldx=None, slope=0.0, upsample=False, res=0, alpha=1.0, beta=1.0, x_std=1.0, wb=None):
    """CPU tensors of one call: x fp16 [B, H, W, ldx] (channels behind cin hold the sentinel), w fp16 [cout, cin, 3, 3], bias fp32, residuals
    fp16 [B, Ho, Wo, cout]."""
    g = _gen(seed)
    ldx = ldx or cin
    x = torch.full((B, H, W, ldx), 0.0, dtype=torch.float16).view(torch.int16).fill_(SENTINEL).view(torch.float16)
    x[..., :cin] = (torch.randn(B, H, W, cin, generator=g) * x_std).half()
    if wb is None:
        w = (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).half()
        bias = torch.randn(cout, generator=g) * 0.1
    else:
        w, bias = wb[0].half(), wb[1].float()
    s = 2 if upsample else 1
    r1 = torch.randn(B, s * H, s * W, cout, generator=g).half() if res >= 1 else None
    r2 = torch.randn(B, s * H, s * W, cout, generator=g).half() if res >= 2 else None
    return dict(x=x, w=w, bias=bias, r1=r1, r2=r2, cin=cin, cout=cout, slope=slope, upsample=upsample, alpha=alpha, beta=beta)


def formula(c, dt):
    """The header's formula in dtype dt on the CPU -> [B, Ho, Wo, cout] (before the output rounding / quantisation)."""
    x = c["x"][..., :c["cin"]].to(dt).permute(0, 3, 1, 2)
    if c["upsample"]:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    y = F.conv2d(x, c["w"].to(dt), c["bias"].to(dt), padding=1).permute(0, 2, 3, 1)
    v = torch.where(y >= 0, y, torch.tensor(c["slope"], dtype=torch.float32).to(dt) * y) if c["slope"] > 0 else y
    if c["r1"] is not None:
        v = torch.tensor(c["alpha"], dtype=torch.float32).to(dt) * v + c["r1"].to(dt)
    if c["r2"] is not None:
        v = torch.tensor(c["beta"], dtype=torch.float32).to(dt) * v + c["r2"].to(dt)
    return v


def device_weight(w, dev):
    """fp16 [npad][9 cin], K order (ky, kx, c), zero rows behind cout -- written here, not taken from ops."""
    cout, cin = w.shape[:2]
    wt = torch.zeros((cout + 15) // 16 * 16, 9 * cin, dtype=torch.float16)
    wt[:cout] = w.permute(0, 2, 3, 1).reshape(cout, 9 * cin)
    return wt.to(dev)


def launch(L, x, ldx, cin, wt, bias, out_ptr, ldo, cout, r1_ptr, ldr1, alpha, r2_ptr, ldr2, beta, slope, upsample, out_mode, B, H, W):
    rc = L.af_dense_conv3x3(x, ldx, cin, wt, bias, out_ptr, ldo, cout, r1_ptr, ldr1, alpha, r2_ptr, ldr2, beta, slope, upsample, out_mode,
                            B, H, W, None)
    torch.cuda.synchronize()
    return rc


def run_fp16(dev, c, out=None, out_ch=0, r2_is_out=False):
    """One call into a fresh sentinel-filled [B, Ho, Wo, cout] tensor (or channels out_ch.. of `out`).  Returns the output tensor on the CPU."""
    from adaface_dev_amd import _lib
    L = _lib.lib()
    x = c["x"].to(dev)
    B, H, W, ldx = x.shape
    s = 2 if c["upsample"] else 1
    if out is None:
        out = torch.empty((B, s * H, s * W, c["cout"]), dtype=torch.int16, device=dev).fill_(SENTINEL).view(torch.float16)
    elif isinstance(out, str):                      # "x": in place
        out = x
    r1 = c["r1"].to(dev) if c["r1"] is not None else None
    r2 = c["r2"].to(dev) if c["r2"] is not None else None
    if r2_is_out:
        out.copy_(r2)
        r2 = out
    p = lambda t: None if t is None else t.data_ptr()
    wt, bias = device_weight(c["w"], dev), c["bias"].to(dev)          # named: they must outlive the call
    rc = launch(L, p(x), ldx, c["cin"], p(wt), p(bias), out.data_ptr() + 2 * out_ch, out.shape[3], c["cout"],
                p(r1), c["cout"], c["alpha"], p(r2), c["cout"], c["beta"], c["slope"], int(c["upsample"]), 0, B, H, W)
    assert rc == 0, L.af_last_error()
    return out.cpu()


def check_bound(got, c, what):
    ref = formula(c, torch.float64)
    e32 = float((formula(c, torch.float32).double() - ref).abs().max())
    bound = 2.0 ** -10 * float(ref.abs().max()) + 4 * e32
    err = float((got.double() - ref).abs().max())
    print(f"{what}: err {err:.3e} bound {bound:.3e} (max|ref| {float(ref.abs().max()):.3f}, e32 {e32:.2e})")
    assert torch.isfinite(got.float()).all()
    assert err <= bound, (what, err, bound)


def test_single_pixel(dev):
    c = make_case(1, 1, 1, 32, 32, seed=1)
    check_bound(run_fp16(dev, c), c, "1x1x1 cin 32 cout 32")


def test_dense_block_write_in_place(dev):
    """cin = 96, cout = 32 written at channels [96, 128) of the ld = 192 buffer it reads: partial patches on both axes, the image boundary inside
    the batch (a halo that read image b's last row for image b + 1's first would show), and every element outside the slice bit for bit."""
    c = make_case(2, 19, 21, 96, 32, seed=2, ldx=192, slope=0.2)
    before = c["x"].clone()
    after = run_fp16(dev, c, out="x", out_ch=96)
    check_bound(after[..., 96:128], c, "2x19x21 in place")
    assert torch.equal(after[..., :96].view(torch.int16), before[..., :96].view(torch.int16))
    assert torch.equal(after[..., 128:].view(torch.int16), before[..., 128:].view(torch.int16))
    assert bool((after[..., 128:].view(torch.int16) == SENTINEL).all())


@pytest.mark.parametrize("hw", [(16, 16), (17, 5)])
def test_two_residuals_r2_aliasing_out(dev, hw):
    c = make_case(1, hw[0], hw[1], 192, 64, seed=3, res=2, alpha=0.2, beta=0.2)
    check_bound(run_fp16(dev, c, r2_is_out=True), c, f"1x{hw[0]}x{hw[1]} cin 192 cout 64 r1 r2")


def test_upsample_odd_source_sides(dev):
    c = make_case(1, 9, 7, 64, 64, seed=4, slope=0.2, upsample=True)
    got = run_fp16(dev, c)
    assert got.shape == (1, 18, 14, 64)
    check_bound(got, c, "1x9x7 upsample")


def test_no_activation_cin_160(dev):
    c = make_case(1, 8, 8, 160, 32, seed=5, slope=0.0)
    assert float(formula(c, torch.float64).min()) < -0.5            # negative outputs survive
    check_bound(run_fp16(dev, c), c, "1x8x8 cin 160 slope 0")


@pytest.mark.parametrize("cout", [16, 24, 40, 48])
def test_output_channel_tiles(dev, cout):
    """One, two and three 16-channel tiles (each count is its own kernel instance), whole and partly filled, with a residual; 18 columns span two
    patches."""
    c = make_case(1, 5, 18, 32, cout, seed=7 + cout, slope=0.2, res=1, alpha=0.2)
    check_bound(run_fp16(dev, c), c, f"1x5x18 cin 32 cout {cout}")


def _u8_case():
    sd = make_state_dict(4, 1, seed=6)
    return make_case(2, 19, 21, 64, 3, seed=6, x_std=0.05, wb=(sd["conv_last.weight"], sd["conv_last.bias"]))


def run_u8(dev, c):
    from adaface_dev_amd import _lib
    L = _lib.lib()
    x = c["x"].to(dev)
    B, H, W, ldx = x.shape
    out = torch.full((B, H, W, c["cout"]), 77, dtype=torch.uint8, device=dev)
    wt, bias = device_weight(c["w"], dev), c["bias"].to(dev)          # named: they must outlive the call
    rc = launch(L, x.data_ptr(), ldx, c["cin"], wt.data_ptr(), bias.data_ptr(), out.data_ptr(), 0, c["cout"],
                None, 0, 1.0, None, 0, 1.0, c["slope"], 0, 1, B, H, W)
    assert rc == 0, L.af_last_error()
    return out.cpu()


def test_uint8_epilogue(dev):
    """cout = 3, out_mode = 1 with conv_last's weights and bias: every value within one level of rint(255 clamp(ref)), and equal wherever 255 ref
    is farther than 255 * 4 e32 from a half-integer.  The share of unclamped elements inside that band must be at most 1 % or the case proves
    nothing (CPU reference: 0.04 % in the band, 13 % of the values clamped)."""
    c = _u8_case()
    ref = formula(c, torch.float64)
    e32 = float((formula(c, torch.float32).double() - ref).abs().max())
    want = torch.round(255 * ref.clamp(0, 1))                                  # torch.round: ties to even
    got = run_u8(dev, c).double()
    s = 255 * ref
    unclamped = (s >= 0) & (s <= 255)
    near = ((s - torch.floor(s) - 0.5).abs() <= 255 * 4 * e32) & unclamped
    share = float(near.sum()) / float(unclamped.sum())
    clamped = 1.0 - float(unclamped.double().mean())
    print(f"uint8: e32 {e32:.2e}, in-band share {share:.4%}, clamped {clamped:.1%}, max level error {float((got - want).abs().max())}")
    assert 0.02 < clamped < 0.5 and float(ref.min()) < -0.05 and float(ref.max()) > 1.05     # both clamps are exercised
    assert share <= 0.01, "inconclusive: too many values at a rounding boundary"
    assert float((got - want).abs().max()) <= 1
    assert torch.equal(got[~near], want[~near])


def test_ops_wrappers_match_the_entry_point(dev):
    from adaface_dev_amd import ops
    c = make_case(2, 19, 21, 96, 32, seed=2, ldx=192, slope=0.2)
    direct = run_fp16(dev, c, out="x", out_ch=96)
    buf = c["x"].to(dev)
    wt = ops.dense_conv3x3_weight(c["w"].to(dev))
    assert torch.equal(wt, device_weight(c["w"], dev))
    ops.dense_conv3x3(buf, 96, wt, c["bias"].to(dev), buf, 96, 32, slope=0.2)
    assert torch.equal(buf.cpu().view(torch.int16), direct.view(torch.int16))
    c = make_case(1, 17, 5, 192, 64, seed=3, res=2, alpha=0.2, beta=0.2)
    direct = run_fp16(dev, c)
    out = torch.zeros((1, 17, 5, 64), dtype=torch.float16, device=dev)
    ops.dense_conv3x3(c["x"].to(dev), 192, ops.dense_conv3x3_weight(c["w"].to(dev)), c["bias"].to(dev), out, 0, 64, r1=c["r1"].to(dev), alpha=0.2,
                      r2=c["r2"].to(dev), beta=0.2)
    assert torch.equal(out.cpu().view(torch.int16), direct.view(torch.int16))
    c = make_case(1, 9, 7, 64, 64, seed=4, slope=0.2, upsample=True)
    out = torch.zeros((1, 18, 14, 64), dtype=torch.float16, device=dev)
    ops.dense_conv3x3(c["x"].to(dev), 64, ops.dense_conv3x3_weight(c["w"].to(dev)), c["bias"].to(dev), out, 0, 64, slope=0.2, upsample=True)
    assert torch.equal(out.cpu().view(torch.int16), run_fp16(dev, c).view(torch.int16))
    c = _u8_case()
    got = ops.dense_conv3x3_u8(c["x"].to(dev), 64, ops.dense_conv3x3_weight(c["w"].to(dev)), c["bias"].to(dev), 3)
    assert torch.equal(got.cpu(), run_u8(dev, c))
    with pytest.raises(RuntimeError, match="output grid"):
        ops.dense_conv3x3(c["x"].to(dev), 64, wt, None, torch.zeros((2, 19, 20, 64), dtype=torch.float16, device=dev), 0, 32)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.dense_conv3x3(c["x"].to(dev), 32, wt, None, c["x"].to(dev), 36, 16)


def test_refusals_leave_the_output_untouched(dev):
    from adaface_dev_amd import _lib
    L = _lib.lib()
    x = torch.zeros((1, 8, 8, 256), dtype=torch.float16, device=dev)
    wt = torch.zeros((80, 9 * 256), dtype=torch.float16, device=dev)
    out = torch.empty((1, 8, 8, 256), dtype=torch.int16, device=dev).fill_(SENTINEL)
    r = torch.zeros((1, 8, 8, 64), dtype=torch.float16, device=dev)
    good = dict(x=x.data_ptr(), ldx=256, cin=64, wt=wt.data_ptr(), out=out.data_ptr(), ldo=256, cout=32, r1=None, r2=None)

    def call(**kw):
        a = dict(good, **kw)
        return launch(L, a["x"], a["ldx"], a["cin"], a["wt"], None, a["out"], a["ldo"], a["cout"], a["r1"], 64, 1.0, a["r2"], 64, 1.0, 0.2, 0, 0,
                      1, 8, 8)

    for kw in (dict(cin=48), dict(cin=224), dict(cout=65), dict(ldx=32), dict(out=x.data_ptr() + 2 * 32, ldo=256), dict(r2=r.data_ptr()),
               dict(x=None), dict(wt=None), dict(out=None)):
        assert call(**kw) == _lib.AF_E_BADARG, kw
        assert b"af_dense_conv3x3" in L.af_last_error()
        assert bool((out == SENTINEL).all()) and bool((x == 0).all())
    assert call() == 0                                               # the same call without a fault goes through
    assert bool((out[..., :32] == 0).all()) and bool((out[..., 32:] == SENTINEL).all())


@pytest.mark.parametrize("r,cpad", [(1, 32), (2, 32), (4, 64), (1, 64)])
def test_u8_unshuffle_is_exact(dev, r, cpad):
    from adaface_dev_amd import ops
    img = torch.randint(0, 256, (2, 8, 12, 3), generator=_gen(r), dtype=torch.uint8)
    img[0, 0, 0], img[1, 7, 11] = torch.tensor([0, 255, 1]), torch.tensor([254, 128, 127])
    ref = F.pixel_unshuffle(img.permute(0, 3, 1, 2).float() / 255, r).permute(0, 2, 3, 1).half()
    got = ops.u8_unshuffle_f16(img.to(dev), r, cpad).cpu()
    assert got.shape == (2, 8 // r, 12 // r, cpad)
    assert torch.equal(got[..., :3 * r * r].view(torch.int16), ref.contiguous().view(torch.int16))
    assert bool((got[..., 3 * r * r:].view(torch.int16) == 0).all())
