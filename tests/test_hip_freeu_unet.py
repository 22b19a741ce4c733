"""FreeU inside the U-Net walk on a real MI355X (`pytest -m gpu`): ``UNetModel.set_freeu`` against a test-side walk that calls the same blocks'
``.hip`` and applies the fp64 restatement of tests/freeu_util.py (rounded to fp16) between them; the off cases bit for bit; beside a ControlNet
(the joined skip is what is filtered) and a motion module."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from controlnet_util import synth_control_images, synth_controlnet_sd
from freeu_util import freeu_ref, to_f16
from motion_util import motion_unet_cfg, synth_motion_sd
from test_hip_unet import GPU_TINY_CONFIG, NET_TOL, _build

pytestmark = pytest.mark.gpu

FREEU = dict(b1=1.5, b2=1.6, s1=0.9, s2=0.2)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def net(dev):
    return _build(GPU_TINY_CONFIG, 11, dev)[0]


def _inputs(dev, side, cc, B=2, seed=71):
    from adaface_dev_amd import ops, rng
    from adaface_dev_amd.ldm.modules.diffusionmodules.util import to_nhwc_f16
    x = rng.synth_input("fu.x", (B, 4, side, side), seed=seed)
    ctx = rng.synth_input("fu.ctx", (B, 77, cc), seed=seed + 1)
    t = torch.tensor([700, 250] * (B // 2))
    return to_nhwc_f16(x.to(dev), ops.round_up(4, 8)), t.to(dev), ctx.to(dev).half().contiguous()


def _hip(unet, x, t, ctx):
    with torch.no_grad():
        e = unet.hip(x, t, ctx)[0]
    torch.cuda.synchronize()
    return e.cpu()


def _hand_walk(unet, x, t, ctx, cfg, control=None):
    """``UNetModel._hip_blocks`` restated with the same blocks' ``.hip``, FreeU between them in fp64 on the CPU (rounded to fp16 once).  With
    ``control`` = (ControlNet, hint, scale) the ControlNet's joins come first, so the joined skip is what is filtered."""
    from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import SkipCat, freeu_plan
    f32 = lambda v: float(np.float32(v))
    with torch.no_grad():
        emb = unet._embed(t)
        kv = unet._project_context_all(ctx)
        try:
            hs, h = [], x
            for m in unet.input_blocks:
                h = m.hip(h, emb, ctx, None)
                hs.append(h)
            if control is not None:
                cn, hint, scale = control
                hs, mid = cn.hip_walk(x, t, ctx, hint, hs, scale, None)
            h = unet.middle_block.hip(h, emb, ctx, None)
            if control is not None:
                h = cn.join_middle(mid, h, scale)
            plan = freeu_plan(unet.model_channels, unet._out_h_channels, cfg)
            assert sum(p is not None for p in plan) >= 4
            for n, m in enumerate(unet.output_blocks):
                skip = hs.pop()
                if plan[n] is not None:
                    rh, rk = freeu_ref(h, skip, f32(plan[n][0]), f32(plan[n][1]), cfg["version"])
                    h, skip = to_f16(rh).to(x.device), to_f16(rk).to(x.device)
                h = m.hip(SkipCat((h, skip)), emb, ctx, None)
            e = unet.out[2].hip(unet.out[0].hip(h, silu=True))
        finally:
            for m in kv:
                m._kv_pre = None
    torch.cuda.synchronize()
    return e.cpu()


@pytest.mark.parametrize("side,version", [(16, 2), (8, 2), (16, 1)])
def test_set_freeu_equals_the_hand_walk(dev, net, side, version):
    """16 x 16 latents, and 8 x 8 so that the 1 x 1 level (one bin, hi == lo) is crossed."""
    x, t, ctx = _inputs(dev, side, GPU_TINY_CONFIG["context_dim"])
    off = _hip(net, x, t, ctx)
    net.set_freeu(**FREEU, version=version)
    try:
        on = _hip(net, x, t, ctx)
        again = _hip(net, x, t, ctx)
        hand = _hand_walk(net, x, t, ctx, dict(FREEU, version=version))
    finally:
        net.set_freeu(None)
    err, effect = rel_l2(on.numpy(), hand.numpy()), rel_l2(on.numpy(), off.numpy())
    print(f"U-Net {side} x {side} with FreeU v{version}: rel-L2 vs the hand walk {err:.3e} (bound {NET_TOL}); on / off differ by {effect:.3e}")
    assert torch.equal(on, again)
    assert effect >= 10 * NET_TOL          # otherwise the comparison shows nothing
    assert err < NET_TOL
    assert torch.equal(_hip(net, x, t, ctx), off)


def test_off_cases_are_bit_identical(dev, net, monkeypatch):
    from adaface_dev_amd import ops
    x, t, ctx = _inputs(dev, 16, GPU_TINY_CONFIG["context_dim"])
    off = _hip(net, x, t, ctx)
    real = ops._launch
    launched = []
    monkeypatch.setattr(ops, "_launch", lambda name, *a, **k: launched.append(name) or real(name, *a, **k))
    _hip(net, x, t, ctx)
    plain, launched[:] = list(launched), []
    net.set_freeu(1, 1, 1, 1)
    try:
        ones = _hip(net, x, t, ctx)
        assert launched == plain and not any("freeu" in n for n in launched)          # the walk launches exactly what it launches unset
    finally:
        net.set_freeu(None)
    assert torch.equal(ones, off)
    launched[:] = []
    assert torch.equal(_hip(net, x, t, ctx), off) and launched == plain
    net.set_freeu(**FREEU)
    try:
        launched[:] = []
        _hip(net, x, t, ctx)
        n_stage = sum(p is not None for p in net.freeu_plan())
        assert [n for n in launched if "freeu" in n] == ["af_freeu_stats", "af_freeu_apply"] * n_stage          # two launches per staged block
        assert [n for n in launched if "freeu" not in n] == plain
    finally:
        net.set_freeu(None)


@pytest.fixture(scope="module")
def wide(dev):
    """(the wrapper tests' reduced-width U-Net, a synthetic ControlNet for it, a synthetic motion module for it) on the device."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.modules.diffusionmodules.controlnet import load_controlnet
    from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    from adaface_dev_amd.ldm.modules.motion_module import MotionModule
    cfg = motion_unet_cfg()
    unet = UNetModel(**cfg)
    rng.load_synth_weights(unet, seed=63)
    return (unet.to(dev).eval(), load_controlnet(synth_controlnet_sd(cfg), cfg).to(dev),
            MotionModule(synth_motion_sd(cfg, with_mid=True, max_len=32, seed=5)).to(dev))


def test_with_a_controlnet_the_joined_skip_is_filtered(dev, wide):
    unet, cn, _ = wide
    x, t, ctx = _inputs(dev, 8, 128)
    with torch.no_grad():
        hint = cn.hint_features(synth_control_images(2, 64, 64).to(dev))
    unet.set_control(cn, hint, 1.0)
    try:
        off = _hip(unet, x, t, ctx)
        unet.set_freeu(**FREEU)
        on = _hip(unet, x, t, ctx)
        hand = _hand_walk(unet, x, t, ctx, dict(FREEU, version=2), control=(cn, hint, 1.0))
        unjoined = _hand_walk(unet, x, t, ctx, dict(FREEU, version=2))
    finally:
        unet.set_freeu(None)
        unet.set_control(None)
    err, effect, join = rel_l2(on.numpy(), hand.numpy()), rel_l2(on.numpy(), off.numpy()), rel_l2(on.numpy(), unjoined.numpy())
    print(f"U-Net + ControlNet with FreeU: rel-L2 vs the hand walk {err:.3e}; on / off differ by {effect:.3e}; without the joins by {join:.3e}")
    assert effect >= 10 * NET_TOL and join >= 10 * NET_TOL
    assert err < NET_TOL


def test_with_a_motion_module(dev, wide):
    unet, _, mm = wide
    nf = 2
    x, t, ctx = _inputs(dev, 8, 128, B=2 * nf)
    unet.set_motion(mm, nf)
    try:
        off = _hip(unet, x, t, ctx)
        unet.set_freeu(**FREEU)
        on = _hip(unet, x, t, ctx)
    finally:
        unet.set_freeu(None)
        unet.set_motion(None)
    effect = rel_l2(on.numpy(), off.numpy())
    print(f"U-Net + motion module with FreeU: on / off differ by {effect:.3e}")
    assert bool(torch.isfinite(on).all()) and effect >= 10 * NET_TOL
