"""af_hint_conv3x3 on a real MI355X (`pytest -m gpu`), through the C entry point (INTEGRATION.md "ControlNet").  The reference is the header's
formula in fp64 on the CPU from the same fp16-rounded (or uint8) inputs and weights; the device weight is written here from the header's
layout, not taken from ops; nothing in the reference comes from the kernel.

Bound per case (fp16 output, the project's own for such a convolution, test_hip_dense_conv.py): 2^-10 max|ref| + 4 e32.  The first term is
one fp16 rounding of the output (2^-11 relative) with room; e32 is the largest error of an fp32 torch CPU evaluation of the whole formula
against fp64 (the kernel accumulates in fp32 too, in another order).

The output is a sentinel-filled tensor of the exact size at the front of a larger allocation whose tail must keep the sentinel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENTINEL = 0x7ABC          # an fp16 bit pattern (finite, 54144.0) no result takes
TAIL = 4096                # elements behind the output that must stay untouched

# (cin, cout, stride) of input_hint_block.{0,2,..,12}; cin 3 is the uint8 image (in_mode 1)
HINT_LAYERS = [(3, 16, 1), (16, 16, 1), (16, 32, 2), (32, 32, 1), (32, 96, 2), (96, 96, 1), (96, 256, 2)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def make_case(B, H, W, cin, cout, stride, seed, act=True, bias=True, x_std=1.0, w_gain=1.0):
    g = torch.Generator().manual_seed(seed)
    if cin == 3:
        x = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.int64).to(torch.uint8)
        x[0, 0, 0, 0], x[0, 0, 0, 1] = 0, 255                       # both ends of the byte range are present
        x[-1, -1, -1, :] = torch.tensor([255, 0, 255], dtype=torch.uint8)
    else:
        x = (torch.randn(B, H, W, cin, generator=g) * x_std).half()
    w = (torch.randn(cout, cin, 3, 3, generator=g) * w_gain / (9 * cin) ** 0.5).half()
    b = torch.randn(cout, generator=g) * 0.1 if bias else None
    return dict(x=x, w=w, bias=b, cin=cin, cout=cout, stride=stride, act=act)


def formula(c, dt):
    """The header's formula in dtype dt on the CPU -> [B, Ho, Wo, cout] (before the output rounding)."""
    x = c["x"].to(dt)
    if c["x"].dtype == torch.uint8:
        x = x / torch.tensor(255.0, dtype=dt)
    y = F.conv2d(x.permute(0, 3, 1, 2), c["w"].to(dt), None if c["bias"] is None else c["bias"].to(dt), stride=c["stride"], padding=1)
    y = y.permute(0, 2, 3, 1)
    return y * torch.sigmoid(y) if c["act"] else y


def device_weight(w, dev):
    """fp16 [cout][9 cpad], index (ky * 3 + kx) * cpad + c, zero for cin <= c < cpad = cin rounded up to 32 -- the header's layout."""
    cout, cin = w.shape[:2]
    cpad = (cin + 31) // 32 * 32
    wt = torch.zeros(cout, 3, 3, cpad, dtype=torch.float16)
    wt[..., :cin] = w.permute(0, 2, 3, 1)
    return wt.reshape(cout, 9 * cpad).to(dev)


def run(dev, c):
    """One call into the front of a sentinel-filled allocation.  Returns (output [B, Ho, Wo, cout], tail) on the CPU."""
    from adaface_dev_amd import _lib
    L = _lib.lib()
    x = c["x"].to(dev)
    B, H, W, _ = x.shape
    s = c["stride"]
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    n = B * Ho * Wo * c["cout"]
    buf = torch.empty(n + TAIL, dtype=torch.int16, device=dev).fill_(SENTINEL)
    wt = device_weight(c["w"], dev)                                  # named: they must outlive the call
    bias = c["bias"].to(dev) if c["bias"] is not None else None
    rc = L.af_hint_conv3x3(x.data_ptr(), int(x.dtype == torch.uint8), c["cin"], wt.data_ptr(), None if bias is None else bias.data_ptr(),
                           buf.data_ptr(), c["cout"], s, int(c["act"]), B, H, W, None)
    torch.cuda.synchronize()
    assert rc == 0, L.af_last_error()
    buf = buf.cpu()
    return buf[:n].view(torch.float16).reshape(B, Ho, Wo, c["cout"]), buf[n:]


def check(dev, c, what):
    got, tail = run(dev, c)
    ref = formula(c, torch.float64)
    assert got.shape == ref.shape
    e32 = float((formula(c, torch.float32).double() - ref).abs().max())
    bound = 2.0 ** -10 * float(ref.abs().max()) + 4 * e32
    err = float((got.double() - ref).abs().max())
    print(f"{what}: err {err:.3e} bound {bound:.3e} (max|ref| {float(ref.abs().max()):.3f}, e32 {e32:.2e})")
    assert bool((tail == SENTINEL).all()), f"{what}: the kernel wrote behind its output"
    assert not bool((got.view(torch.int16) == SENTINEL).any()), f"{what}: an output element was not written"
    assert torch.isfinite(got.float()).all()
    assert err <= bound, (what, err, bound)
    return ref


@pytest.mark.parametrize("cin,cout,stride", HINT_LAYERS, ids=[f"{a}to{b}_s{s}" for a, b, s in HINT_LAYERS])
def test_hint_encoder_layers_odd_size(dev, cin, cout, stride):
    """B = 2, 19 x 21: partial tiles on both axes, the image boundary inside the batch, and at stride 2 a 10 x 11 output whose last row and
    column read the zero border."""
    c = make_case(2, 19, 21, cin, cout, stride, seed=10 + cout + stride)
    ref = check(dev, c, f"2x19x21 {cin}->{cout} s{stride}")
    assert ref.shape[1:3] == ((10, 11) if stride == 2 else (19, 21))


def test_stride2_even_size(dev):
    check(dev, make_case(2, 20, 24, 32, 96, 2, seed=3), "2x20x24 32->96 s2")


def test_stride2_one_fragment(dev):
    """16 -> 16 at stride 2: the kernel instance (stride 2, one fragment per slab) that no layer of the hint encoder runs.  On the CPU:
    max|ref| 3.4, e32 1.1e-6, in the range of the neighbouring 16-channel cases (3.9 .. 4.5, 1.7e-6)."""
    ref = check(dev, make_case(2, 19, 21, 16, 16, 2, seed=13), "2x19x21 16->16 s2")
    assert ref.shape == (2, 10, 11, 16)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 37)])
@pytest.mark.parametrize("stride", [1, 2])
def test_thin_images(dev, H, W, stride):
    check(dev, make_case(1, H, W, 16, 32, stride, seed=4 + W), f"1x{H}x{W} 16->32 s{stride}")


def test_several_tiles_all_fragments(dev):
    """40 x 72 at 96 -> 256 stride 2: 20 x 36 outputs = 3 x 3 patches of 8 x 16, four channel slabs of four fragments."""
    check(dev, make_case(1, 40, 72, 96, 256, 2, seed=5), "1x40x72 96->256 s2")


@pytest.mark.parametrize("cin,cout", [(256, 16), (16, 256)])
def test_corners_of_the_range(dev, cin, cout):
    check(dev, make_case(1, 19, 21, cin, cout, 1, seed=6 + cin), f"1x19x21 {cin}->{cout} s1")


def test_act_off(dev):
    c = make_case(2, 19, 21, 32, 32, 1, seed=7, act=False)
    ref = check(dev, c, "act off")
    assert float(ref.min()) < -0.3                                  # a SiLU left on would show: SiLU's minimum is -0.278


def test_silu_tails(dev):
    """Inputs scaled so that |y| reaches ~20: sigmoid saturates on both sides."""
    c = make_case(2, 19, 21, 32, 32, 1, seed=8, x_std=6.0)
    y = formula(dict(c, act=False), torch.float64)
    assert float(y.max()) > 18 and float(y.min()) < -18
    check(dev, c, "SiLU tails")


def test_bias_null(dev):
    check(dev, make_case(2, 19, 21, 16, 16, 1, seed=9, bias=False), "bias NULL")
    check(dev, make_case(1, 9, 11, 3, 16, 1, seed=9, bias=False), "bias NULL, uint8 image")


def test_u8_image_extremes(dev):
    """in_mode 1 on an image of 0 and 255 only (with single pixels of the other value), against the same formula."""
    c = make_case(2, 16, 24, 3, 16, 1, seed=11)
    x = torch.zeros_like(c["x"])
    x[:, 4:12, 6:18] = 255
    x[0, 0, 0, 1] = 255
    x[1, 8, 8, 2] = 0
    c["x"] = x
    assert set(np.unique(x.numpy()).tolist()) == {0, 255}
    check(dev, c, "uint8 0 / 255")


def test_ops_wrapper_matches_the_entry_point(dev):
    """ops.pack_hint_conv3x3 writes the header's layout and ops.hint_conv3x3 is the same launch."""
    from adaface_dev_amd import ops
    c = make_case(2, 19, 21, 16, 32, 2, seed=12)
    assert torch.equal(ops.pack_hint_conv3x3(c["w"]), device_weight(c["w"], "cpu"))
    got, _ = run(dev, c)
    out = ops.hint_conv3x3(c["x"].to(dev), ops.pack_hint_conv3x3(c["w"].to(dev)), c["bias"].to(dev), stride=2, act=True)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), got)
