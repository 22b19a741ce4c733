"""Nearest x2 + 3x3 convolution as four 2x2 phase convolutions of the low-res image (af_gemm_desc.upsample = 3, ops.pack_conv3x3_up2 /
ops.conv3x3_up2, Conv2d.hip(upsample=True)): the weight folding on the CPU, the kernel against torch, every output element at its place, and the
scope outside which Conv2d.hip keeps the nine-tap gather."""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

TOL = 2e-3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()  # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.float16)


def up2_ref(x_nhwc, w, bias=None):
    """F.interpolate nearest + F.conv2d in the inputs' float dtype (fp16 inputs: fp32); NCHW result."""
    dt = torch.float64 if x_nhwc.dtype == torch.float64 else torch.float32
    xin = x_nhwc.to(dt).permute(0, 3, 1, 2)
    return F.conv2d(F.interpolate(xin, scale_factor=2, mode="nearest"), w.to(dt), None if bias is None else bias.to(dt), padding=1)


# ------------------------------------------------------------------------------- the pack, no GPU
def test_phase_weights_follow_the_folding_formula():
    """Tap i of output row 2y + py reads source row y + floor((py + i - 1) / 2): weight (a, b) of phase (py, px) is the sum of the 3x3 weights
    whose taps land on offset (py - 1 + a, px - 1 + b)."""
    from adaface_dev_amd import ops
    w = torch.randn((5, 3, 3, 3), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    got = ops.up2_phase_weights(w)
    assert got.shape == (4, 5, 2, 2, 3) and got.dtype == torch.float64
    want = torch.zeros_like(got)
    for py in range(2):
        for px in range(2):
            for i in range(3):
                for j in range(3):
                    a, b = (py + i - 1) // 2 - (py - 1), (px + j - 1) // 2 - (px - 1)
                    want[2 * py + px, :, a, b, :] += w[:, :, i, j]
    assert torch.equal(got, want) or float((got - want).abs().max()) < 1e-15
    # py = 0: {w0, w1 + w2}; py = 1: {w0 + w1, w2}
    assert torch.allclose(got[0, :, 1, 1], (w[:, :, 1:, 1:]).sum((2, 3)), atol=1e-15, rtol=0)
    assert torch.allclose(got[3, :, 0, 0], (w[:, :, :2, :2]).sum((2, 3)), atol=1e-15, rtol=0)
    assert torch.equal(got[0, :, 0, 0], w[:, :, 0, 0]) and torch.equal(got[3, :, 1, 1], w[:, :, 2, 2])


def test_four_phase_convolutions_equal_interpolate_conv_in_fp64():
    from adaface_dev_amd import ops
    g = torch.Generator().manual_seed(2)
    B, H, W, cin, cout = 2, 5, 6, 3, 4
    x = torch.randn((B, H, W, cin), generator=g, dtype=torch.float64)
    w = torch.randn((cout, cin, 3, 3), generator=g, dtype=torch.float64)
    ref = up2_ref(x, w)
    wp = ops.up2_phase_weights(w)
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1))                      # the zero padding of the hi-res grid is that of the low-res grid
    out = torch.empty_like(ref)
    for py in range(2):
        for px in range(2):
            y = F.conv2d(xp, wp[2 * py + px].permute(0, 3, 1, 2))        # [B, cout, H + 1, W + 1]: offsets {py - 1, py} start at padded row y + py
            out[:, :, py::2, px::2] = y[:, :, py:py + H, px:px + W]
    assert float((out - ref).abs().max()) < 1e-12


def test_pack_layout_and_single_rounding():
    """Rows [4 Cout] phase-major, K (a, b, cin), the fp32 sums rounded to fp16 once; the bias stays [Cout]."""
    from adaface_dev_amd import ops
    cout, cin = 160, 64
    w = torch.randn((cout, cin, 3, 3), generator=torch.Generator().manual_seed(3)) * (9 * cin) ** -0.5
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(4))
    pw = ops.pack_conv3x3_up2(w, bias, "cpu")
    assert (pw.N, pw.K, pw.kpad, pw.taps, pw.cin, pw.up2) == (cout, 4 * cin, 4 * cin, 9, cin, True)
    assert pw.wt.shape == (4 * cout, 4 * cin) and pw.wt.dtype == torch.float16 and torch.equal(pw.bias, bias)
    want = ops.up2_phase_weights(w).reshape(4 * cout, 4 * cin).to(torch.float16)
    assert torch.equal(pw.wt, want)
    assert torch.equal(pw.wt[3 * cout + 7, (1 * 2 + 1) * cin + 5], w[7, 5, 2, 2].to(torch.float16))


# ------------------------------------------------------------------------------- the kernel
SHAPES = [(2, 16, 16, 64, 160),       # one chunk (first == last), one image per tile
          (1, 32, 32, 128, 320),      # 8-row tiles: top border, interior, bottom border; two chunks (halo buffer swap); two N tiles per phase
          (2, 16, 16, 192, 160),      # three chunks: the ring slot wraps across chunk boundaries
          (1, 32, 32, 640, 640)]      # the real channel count at one image


@functools.lru_cache(maxsize=None)
def case(B, H, W, cin, cout):
    """Inputs and the fp32 torch reference WITHOUT bias (shared by the bias-on and bias-off cases; never modified)."""
    x = rnd((B, H, W, cin), 1)
    w = rnd((cout, cin, 3, 3), 3, (9 * cin) ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(4))
    return x, w, bias, up2_ref(x, w)


@pytest.mark.gpu
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("B,H,W,cin,cout", SHAPES)
def test_phase_kernel_against_torch_and_the_nine_tap_kernel(dev, B, H, W, cin, cout, with_bias):
    from adaface_dev_amd import ops
    x, w, bias, ref = case(B, H, W, cin, cout)
    b = bias if with_bias else None
    if with_bias:
        ref = ref + bias[None, :, None, None]
    d = ops.conv_up2_desc(B, H, W, cin, cout)
    assert ops.conv_up2_eligible(d)
    pw, pw9 = ops.pack_conv3x3_up2(w, b, dev), ops.pack_conv3x3(w, b, dev)
    xd = x.to(dev)
    out = ops.conv3x3_up2(xd, pw)
    assert out.shape == (B, 2 * H, 2 * W, cout)
    e_ref = rel_l2(out.float().cpu().permute(0, 3, 1, 2).numpy(), ref.numpy())
    old = ops.conv3x3(xd, pw9, upsample=True, tile=14, splits=1)
    e_old = rel_l2(out.float().cpu().numpy(), old.float().cpu().numpy())
    print(f"up2 phase {(B, H, W, cin, cout)} bias={with_bias}: rel_l2 vs fp32 torch {e_ref:.3e}, vs nine-tap tile 14 {e_old:.3e}")
    assert e_ref < TOL
    assert e_old < 2e-3
    for _ in range(5):
        assert torch.equal(ops.conv3x3_up2(xd, pw), out)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,cin,cout", SHAPES[:2])
def test_every_output_element_is_written_at_its_place(dev, B, H, W, cin, cout):
    """x = 0 and a distinct bias per channel: every pixel of the (NaN-filled) output must hold bias[n] bit-exactly."""
    from adaface_dev_amd import ops
    w = rnd((cout, cin, 3, 3), 3, (9 * cin) ** -0.5)
    bias = torch.arange(1, cout + 1, dtype=torch.float32)                 # exact in fp16
    out = ops.conv3x3_up2(torch.zeros((B, H, W, cin), dtype=torch.float16, device=dev), ops.pack_conv3x3_up2(w, bias, dev))
    assert torch.equal(out.cpu(), bias.to(torch.float16).expand(B, 2 * H, 2 * W, cout))


@pytest.mark.gpu
@pytest.mark.parametrize("y,x", [(0, 0), (31, 31), (7, 18), (8, 0)])
def test_single_low_res_pixel_lands_on_its_4x4_footprint(dev, y, x):
    """One non-zero low-res pixel (corners, a tile's first row, an interior one): the 4 x 4 output footprint matches the reference, the rest is 0."""
    from adaface_dev_amd import ops
    B, H, W, cin, cout = 1, 32, 32, 128, 320
    w = rnd((cout, cin, 3, 3), 3, (9 * cin) ** -0.5)
    xs = torch.zeros((B, H, W, cin), dtype=torch.float16)
    xs[0, y, x] = rnd((cin,), 5)
    ref = up2_ref(xs, w)
    out = ops.conv3x3_up2(xs.to(dev), ops.pack_conv3x3_up2(w, None, dev)).float().cpu().permute(0, 3, 1, 2)
    assert rel_l2(out.numpy(), ref.numpy()) < TOL
    foot = torch.zeros((2 * H, 2 * W), dtype=torch.bool)
    foot[max(2 * y - 1, 0):2 * y + 3, max(2 * x - 1, 0):2 * x + 3] = True
    assert torch.equal((ref != 0).any(1)[0], foot)                        # (the reference's own support: the test's geometry)
    assert bool((out[0][:, ~foot] == 0).all())


# ------------------------------------------------------------------------------- scope
def make_conv(cin, cout, dev):
    from adaface_dev_amd.ldm.modules.diffusionmodules.util import Conv2d
    conv = Conv2d(cin, cout, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(rnd((cout, cin, 3, 3), 3, (9 * cin) ** -0.5).float())
        conv.bias.copy_(torch.randn(cout, generator=torch.Generator().manual_seed(4)))
    return conv.to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("what,B,H,W,c1,c2,cout", [("8x8", 2, 8, 8, 64, 0, 160), ("cout128", 2, 16, 16, 64, 0, 128), ("second source", 2, 16, 16, 64, 64, 160),
                                                   ("residual", 2, 16, 16, 64, 0, 160)])
def test_outside_the_scope_conv2d_keeps_the_nine_tap_path(dev, what, B, H, W, c1, c2, cout):
    from adaface_dev_amd import ops
    conv = make_conv(c1 + c2, cout, dev)
    x1, x2 = rnd((B, H, W, c1), 1), (rnd((B, H, W, c2), 2) if c2 else None)
    res = rnd((B, 2 * H, 2 * W, cout), 6) if what == "residual" else None
    xd, x2d, resd = x1.to(dev), None if x2 is None else x2.to(dev), None if res is None else res.to(dev)
    assert not ops.conv_up2_eligible(ops.conv_up2_desc(B, H, W, c1, cout, c2=c2, residual=resd))
    out = conv.hip(xd, x2=x2d, upsample=True, residual=resd)
    today = ops.conv3x3(xd, conv.packed(), x2=x2d, upsample=True, residual=resd)
    assert torch.equal(out, today)
    ref = up2_ref(x1 if x2 is None else torch.cat([x1, x2], -1), conv.weight.detach().cpu(), conv.bias.detach().cpu())
    if res is not None:
        ref = ref + res.float().permute(0, 3, 1, 2)
    assert rel_l2(out.float().cpu().permute(0, 3, 1, 2).numpy(), ref.numpy()) < TOL


@pytest.mark.gpu
def test_split_k_is_outside_the_scope_and_refused(dev):
    """splits = 2: the predicate says no and the library refuses the launch; Conv2d.hip (which never splits this form) is right and, with the
    form switched off, bit-identical to the nine-tap path."""
    from adaface_dev_amd import ops
    B, H, W, cin, cout = 2, 16, 16, 128, 160
    assert ops.conv_up2_eligible(ops.conv_up2_desc(B, H, W, cin, cout))
    assert not ops.conv_up2_eligible(ops.conv_up2_desc(B, H, W, cin, cout, splits=2))
    conv = make_conv(cin, cout, dev)
    x = rnd((B, H, W, cin), 1)
    xd = x.to(dev)
    with pytest.raises(RuntimeError, match="upsample = 3"):
        ops.conv3x3_up2(xd, conv.packed_up2(), splits=2)
    with pytest.raises(RuntimeError, match="upsample = 3"):
        ops.conv3x3_up2(xd, conv.packed_up2(), tile=11)                   # no other tile reads the phase pack
    out = conv.hip(xd, upsample=True)
    ref = up2_ref(x, conv.weight.detach().cpu(), conv.bias.detach().cpu())
    assert rel_l2(out.float().cpu().permute(0, 3, 1, 2).numpy(), ref.numpy()) < TOL


@pytest.mark.gpu
def test_switch_off_gives_the_nine_tap_result_bit_for_bit(dev, monkeypatch):
    from adaface_dev_amd import ops
    B, H, W, cin, cout = 2, 16, 16, 128, 160
    conv = make_conv(cin, cout, dev)
    xd = rnd((B, H, W, cin), 1).to(dev)
    today = ops.conv3x3(xd, conv.packed(), upsample=True)
    monkeypatch.setenv("AF_UP2_PHASE", "0")
    assert torch.equal(conv.hip(xd, upsample=True), today)
    monkeypatch.setenv("AF_UP2_PHASE", "1")
    on = conv.hip(xd, upsample=True)
    assert torch.equal(on, ops.conv3x3_up2(xd, conv.packed_up2()))        # the phase form ran
    assert rel_l2(on.float().cpu().numpy(), today.float().cpu().numpy()) < 2e-3
