"""The phase form of nearest x2 + 3x3 at the 8 x 8 level (af_gemm_halo_variant 5): the whole-line tap-by-tap kernel walks the low-res image with
the four taps of its N tile's phase under split-K, and af_splitk_reduce_kernel sums the fp32 slabs straight into the hi-res tensor.  Against fp32
torch with the nine-tap launch's own error as the yardstick; bitwise repeatable; every output element written, no lane outside the image read."""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

TILES = (7, 8, 11, 12, 13)            # the whole-line tiles the form may be asked for (the library decides which it takes at a width)
SPLITS = (1, 2, 4)


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


@functools.lru_cache(maxsize=None)
def case(B, cin, cout):
    """Input, weights, bias and the fp32 torch reference F.conv2d(F.interpolate(x, 2, 'nearest')) (NCHW; never modified)."""
    x = rnd((B, 8, 8, cin), 1)
    w = rnd((cout, cin, 3, 3), 3, (9 * cin) ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(4))
    ref = F.conv2d(F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2, mode="nearest"), w.float(), bias, padding=1)
    return x, w, bias, ref.numpy()


def configs(ops, B, cin, cout):
    """Every (tile, splits) of the sweep the library's predicate takes at this shape."""
    return [(t, s) for t in TILES for s in SPLITS if ops.conv_up2_eligible(ops.conv_up2_desc(B, 8, 8, cin, cout, tile=t, splits=s))]


def test_scope_of_the_8x8_form():
    """Host side of the predicate: split-K is required, the tile's width must divide Cout, K slices of at least one 64-wide stage, 8 x 8 only."""
    from adaface_dev_amd import ops
    el = lambda *a, **k: ops.conv_up2_eligible(ops.conv_up2_desc(*a, **k))
    assert el(8, 8, 8, 1280, 1280, tile=13, splits=4) and el(8, 8, 8, 1280, 1280, tile=7, splits=2) and el(8, 8, 8, 1280, 1280, tile=8, splits=8)
    assert not el(8, 8, 8, 1280, 1280, tile=13, splits=1)             # unsplit: the kernel's own epilogue has no phase map
    assert not el(8, 8, 8, 1280, 1280, tile=14, splits=4)             # the halo-resident kernel does not take the level
    assert not el(2, 8, 8, 64, 160, tile=7, splits=2)                 # 320 does not divide 160: an N tile would straddle two phases
    assert not el(2, 8, 8, 64, 160, tile=8, splits=2)
    assert el(2, 8, 8, 64, 160, tile=11, splits=4) and not el(2, 8, 8, 64, 160, tile=11, splits=8)      # K = 256: four stages
    assert not el(2, 16, 16, 64, 160, tile=11, splits=2)              # the other levels stay on tile 14
    assert not el(2, 8, 8, 64, 160, tile=11, splits=2, c2=64)
    assert configs(ops, 3, 64, 160) == [(11, 2), (11, 4), (13, 2), (13, 4)]
    assert ops.conv_up2_config(8, 8, 8, 1280, 1280)[1] >= 2 and ops.conv_up2_config(2, 8, 8, 64, 160) == (14, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 4, 8])
@pytest.mark.parametrize("cin,cout", [(64, 160), (128, 320)])
def test_8x8_phase_form_against_torch(dev, B, cin, cout):
    """B = 1, 3 leave a 128-row tile partly empty, 4 fills tiles exactly, 8 is the workload's batch.  Tolerance: the nine-tap launch's measured
    error on the same input x 1.5.  Poisoned output and NaN rows around the input: every hi-res element is written, no out-of-image lane is read.
    20 launches bitwise equal."""
    from adaface_dev_amd import ops
    x, w, bias, ref = case(B, cin, cout)
    pw, pw9 = ops.pack_conv3x3_up2(w, bias, dev), ops.pack_conv3x3(w, bias, dev)
    # the input in the middle of a NaN-filled buffer (16-byte aligned): a gather that leaves the images reads NaN
    n, pad = x.numel(), 4 * 8 * cin
    buf = torch.full((n + 2 * pad,), float("nan"), dtype=torch.float16, device=dev)
    buf[pad:pad + n] = x.reshape(-1).to(dev)
    xd = buf[pad:pad + n].view(B, 8, 8, cin)
    nine = ops.conv3x3(x.to(dev), pw9, upsample=True)
    tol = 1.5 * rel_l2(nine.float().cpu().permute(0, 3, 1, 2).numpy(), ref)
    cfgs = configs(ops, B, cin, cout)
    assert {s for _, s in cfgs} == {2, 4} and len({t for t, _ in cfgs}) >= 2
    for tile, splits in cfgs:
        out = torch.full((B, 16, 16, cout), float("nan"), dtype=torch.float16, device=dev)
        assert ops.conv3x3_up2(xd, pw, tile=tile, splits=splits, out=out) is out
        assert not bool(torch.isnan(out).any()), (tile, splits)
        err = rel_l2(out.float().cpu().permute(0, 3, 1, 2).numpy(), ref)
        print(f"up2 8x8 B={B} {cin}->{cout} tile {tile} x{splits}: rel_l2 vs fp32 torch {err:.3e} (nine-tap x 1.5 = {tol:.3e})")
        assert err <= tol, (tile, splits)
        for _ in range(20):
            assert torch.equal(ops.conv3x3_up2(xd, pw, tile=tile, splits=splits), out), (tile, splits)
    with pytest.raises(RuntimeError, match="upsample = 3"):
        ops.conv3x3_up2(xd, pw, tile=cfgs[0][0], splits=1)


@pytest.mark.gpu
def test_production_shape_against_the_nine_tap_launch(dev, monkeypatch):
    """8 x 8 x 8, 1280 -> 1280: the measured configuration (and one of every other tile) against fp32 torch, tolerance = the nine-tap launch's
    measured error x 1.5; with AF_UP2_PHASE_8X8=1 Conv2d.hip takes the form at this shape."""
    monkeypatch.setenv("AF_UP2_PHASE_8X8", "1")
    from adaface_dev_amd import ops
    from adaface_dev_amd.ldm.modules.diffusionmodules.util import Conv2d
    B, c = 8, 1280
    x, w, bias, ref = case(B, c, c)
    conv = Conv2d(c, c, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(w.float())
        conv.bias.copy_(bias)
    conv = conv.to(dev)
    xd = x.to(dev)
    nine = ops.conv3x3(xd, conv.packed(), upsample=True)
    tol = 1.5 * rel_l2(nine.float().cpu().permute(0, 3, 1, 2).numpy(), ref)
    shipped = ops.conv_up2_config(B, 8, 8, c, c)
    assert ops.conv_up2_eligible(ops.conv_up2_desc(B, 8, 8, c, c, tile=shipped[0], splits=shipped[1]))
    for tile, splits in [shipped] + [(t, 4) for t in TILES if t != shipped[0]]:
        out = torch.full((B, 16, 16, c), float("nan"), dtype=torch.float16, device=dev)
        ops.conv3x3_up2(xd, conv.packed_up2(), tile=tile, splits=splits, out=out)
        err = rel_l2(out.float().cpu().permute(0, 3, 1, 2).numpy(), ref)
        print(f"up2 8x8 production tile {tile} x{splits}: rel_l2 vs fp32 torch {err:.3e} (nine-tap x 1.5 = {tol:.3e})")
        assert not bool(torch.isnan(out).any()) and err <= tol, (tile, splits)
        if (tile, splits) == shipped:
            assert torch.equal(conv.hip(xd, upsample=True), out)


@pytest.mark.gpu
def test_8x8_level_is_on_the_nine_taps_unless_switched_on(dev, monkeypatch):
    """The level's phase form is off by default (its gain in the step did not clear the run-to-run spread); AF_UP2_PHASE=0 overrides AF_UP2_PHASE_8X8=1."""
    from adaface_dev_amd import ops
    from adaface_dev_amd.ldm.modules.diffusionmodules.util import Conv2d
    B, c = 8, 1280
    x, w, bias, _ = case(B, c, c)
    conv = Conv2d(c, c, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(w.float())
        conv.bias.copy_(bias)
    conv = conv.to(dev)
    xd = x.to(dev)
    nine = ops.conv3x3(xd, conv.packed(), upsample=True)
    monkeypatch.delenv("AF_UP2_PHASE_8X8", raising=False)
    assert torch.equal(conv.hip(xd, upsample=True), nine)
    monkeypatch.setenv("AF_UP2_PHASE_8X8", "1")
    assert not torch.equal(conv.hip(xd, upsample=True), nine)
    monkeypatch.setenv("AF_UP2_PHASE", "0")
    assert torch.equal(conv.hip(xd, upsample=True), nine)
