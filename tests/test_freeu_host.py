"""FreeU on the host: the closed form of the skip low-pass against the authors' ``torch.fft`` composition, the per-output-block plan, the
validation of ``UNetModel.set_freeu`` / ``AdaFaceWrapper.enable_freeu`` / the constructor, and the refusals by name.  Nothing here needs a GPU."""
import numpy as np
import pytest
import torch

from adaface_dev_amd import TINY_UNET_CONFIG
from adaface_dev_amd.adaface.adaface_wrapper import SD15_UNET_CONFIG, AdaFaceWrapper
from adaface_dev_amd.adaface.arc2face_models import clip_text_config
from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel, check_freeu_values, freeu_plan
from freeu_util import bins, boost_factor, fourier_filter_fft, freeu_ref, lowpass_closed

SIZES = [(1, 1), (1, 4), (2, 1), (2, 2), (3, 5), (5, 3), (4, 2), (7, 7), (8, 8), (16, 24)]
SCALES = [0.0, 0.2, 0.9, 1.0, 2.5]


# ---------------------------------------------------------------------------------------------------------------- closed form
@pytest.mark.parametrize("H,W", SIZES)
def test_closed_form_equals_the_fft_composition(H, W):
    g = torch.Generator().manual_seed(100 * H + W)
    x = torch.randn((2, 3, H, W), generator=g, dtype=torch.float64)
    for s in SCALES:
        ref = fourier_filter_fft(x, 1, s).permute(0, 2, 3, 1).numpy()
        got = lowpass_closed(x.permute(0, 2, 3, 1).numpy(), s)
        err = float(np.abs(got - ref).max())
        assert err < 1e-12, (H, W, s, err)


def test_bins_and_the_swaps_that_matter():
    assert bins(1, 1) == [(0, 0)] and bins(1, 4) == [(0, 0), (0, -1)] and bins(2, 1) == [(0, 0), (-1, 0)] and len(bins(3, 5)) == 4
    g = torch.Generator().manual_seed(7)
    x = torch.randn((1, 5, 7, 2), generator=g, dtype=torch.float64).numpy()          # NHWC: 5 x 7 pixels
    good = lowpass_closed(x, 0.2)
    # the conjugate of the diagonal bin gives the same real part, (-1, +1) does not; a dropped bin shows
    assert np.abs(lowpass_closed(x, 0.2, diag_v=+1) - good).max() > 1e-3
    assert np.abs(lowpass_closed(x, 0.2, drop=(-1, 0)) - good).max() > 1e-3
    ref = fourier_filter_fft(torch.from_numpy(x).permute(0, 3, 1, 2), 1, 0.2).permute(0, 2, 3, 1).numpy()
    assert np.abs(good - ref).max() < 1e-12


def test_boost_rule():
    h = np.zeros((2, 2, 2, 4))
    h[0, :, :, :] = np.array([[1.0, 2.0], [3.0, 5.0]])[:, :, None]          # sample 0: means 1, 2, 3, 5
    h[1] = 7.0                                                               # sample 1: constant mean, hi == lo -> mhat = 0
    f = boost_factor(h, 1.5, 2)
    assert np.allclose(f[0, :, :, 0], 1 + 0.5 * np.array([[0.0, 0.25], [0.5, 1.0]])) and np.all(f[1] == 1.0)
    assert np.all(boost_factor(h, 1.5, 1) == 1.5)
    ho, ko = freeu_ref(np.full((1, 1, 1, 4), 60000.0, np.float16), np.ones((1, 1, 1, 8), np.float16), 1.5, 1.0, version=1)
    assert np.all(ho[..., :2] == 65504.0) and np.all(ho[..., 2:] == 60000.0) and np.all(ko == 1.0)


# ---------------------------------------------------------------------------------------------------------------- plan
def _h_channels(cfg):
    with torch.device("meta"):
        return UNetModel(**cfg)


def test_plan_sd15():
    m = _h_channels(SD15_UNET_CONFIG)
    assert m.model_channels == 320 and len(m.output_blocks) == 12
    assert m._out_h_channels == [1280] * 7 + [640] * 3 + [320] * 2
    assert m.freeu_plan() == [None] * 12
    m.set_freeu(1.5, 1.6, 0.9, 0.2)
    assert m.freeu_plan() == [(1.5, 0.9)] * 7 + [(1.6, 0.2)] * 3 + [None] * 2
    m.set_freeu(None)
    assert m.freeu_plan() == [None] * 12


def test_plan_tiny():
    from test_hip_unet import GPU_TINY_CONFIG
    m = _h_channels(GPU_TINY_CONFIG)
    assert m.model_channels == 64
    cfg = check_freeu_values("t", 1.5, 1.6, 0.9, 0.2, 2)
    plan = freeu_plan(64, m._out_h_channels, cfg)
    staged = {c: p for c, p in zip(m._out_h_channels, plan)}
    assert staged[256] == (1.5, 0.9) and staged[128] == (1.6, 0.2) and staged.get(64) is None
    assert 256 in staged and 128 in staged
    assert freeu_plan(64, m._out_h_channels, None) == [None] * len(m.output_blocks)


# ---------------------------------------------------------------------------------------------------------------- validation, refusals
def _tiny_unet():
    return UNetModel(**dict(TINY_UNET_CONFIG))


BAD = [dict(b1=-1.0), dict(b2=float("nan")), dict(s1=float("inf")), dict(s2=-0.1), dict(version=3), dict(b1="1.5"), dict(version=True)]


@pytest.mark.parametrize("bad", BAD)
def test_set_freeu_validates(bad):
    m = _tiny_unet()
    kw = dict(b1=1.5, b2=1.6, s1=0.9, s2=0.2, version=2)
    kw.update(bad)
    with pytest.raises(ValueError, match=next(iter(bad))):
        m.set_freeu(**kw)
    assert m._freeu is None


def test_state_dict_unchanged_and_refusals_by_name():
    m = _tiny_unet()
    keys = list(m.state_dict().keys())
    m.set_freeu(1.5, 1.6, 0.9, 0.2, version=1)
    assert m._freeu == dict(b1=1.5, b2=1.6, s1=0.9, s2=0.2, version=1)
    assert list(m.state_dict().keys()) == keys and "_freeu" not in m._modules and "_freeu" not in m._parameters and "_freeu" not in m._buffers
    x = torch.zeros(1, 4, 8, 8, requires_grad=True)
    ctx = torch.zeros(1, 77, m._cross_attn_layers()[0].to_k.in_features)
    t = torch.tensor([1])
    calls = {
        "hip_train": lambda: m.hip_train(None, None, None),
        "hip_train_trunk": lambda: m.hip_train_trunk(None, None, None, None, 3),
        "hip_trunk": lambda: m.hip_trunk(None, None, None, None, 3),
        "hip_tail": lambda: m.hip_tail((None, None), None, None, ()),
        "hip_bwd": lambda: m.hip_bwd(None, None),
        "hip_bwd_trunk": lambda: m.hip_bwd_trunk(None, None, []),
        "training": lambda: m(x, t, ctx, extra_info={}),
        "score-rewrite": lambda: m(x.detach(), t, ctx, extra_info={"normalize_cross_attn": True}),
    }
    for what, call in calls.items():
        with pytest.raises(NotImplementedError, match="FreeU") as e:
            call()
        assert what in str(e.value), (what, str(e.value))
    m.set_freeu(None)
    assert m._freeu is None


def _wrapper(pipeline_name="text2img", **kw):
    cc = clip_text_config(hidden_size=64, num_attention_heads=1, num_hidden_layers=1, intermediate_size=128)
    return AdaFaceWrapper(pipeline_name=pipeline_name, clip_config=cc, unet_config=dict(TINY_UNET_CONFIG, context_dim=64), device="cpu", **kw)


def test_wrapper_enable_disable_and_constructor():
    w = _wrapper()
    unet = w.ldm.model.diffusion_model
    assert w.freeu is None and unet._freeu is None
    assert w.enable_freeu() == dict(b1=1.5, b2=1.6, s1=0.9, s2=0.2, version=2)          # the authors' SD-1.5 values; diffusers' argument order
    assert unet._freeu == w.freeu == dict(b1=1.5, b2=1.6, s1=0.9, s2=0.2, version=2)
    w.enable_freeu(0.8, 0.3, 1.2, 1.3, version=1)
    assert unet._freeu == dict(b1=1.2, b2=1.3, s1=0.8, s2=0.3, version=1)
    for bad in BAD:
        with pytest.raises(ValueError, match=next(iter(bad))):
            w.enable_freeu(**bad)
        assert unet._freeu == dict(b1=1.2, b2=1.3, s1=0.8, s2=0.3, version=1)             # a refused call changes nothing
    w.disable_freeu()
    assert w.freeu is None and unet._freeu is None
    assert _wrapper(freeu=True).ldm.model.diffusion_model._freeu == dict(b1=1.5, b2=1.6, s1=0.9, s2=0.2, version=2)
    assert _wrapper(freeu=dict(b1=1.1, s2=0.5)).ldm.model.diffusion_model._freeu == dict(b1=1.1, b2=1.6, s1=0.9, s2=0.5, version=2)
    assert _wrapper(freeu=None).ldm.model.diffusion_model._freeu is None
    with pytest.raises(ValueError, match="b3"):
        _wrapper(freeu=dict(b3=1.0))
    with pytest.raises(ValueError, match="version"):
        _wrapper(freeu=dict(version=3))
    with pytest.raises(ValueError, match="freeu must be"):
        _wrapper(freeu=1.5)


def test_wrapper_without_a_unet_refuses():
    with pytest.raises(RuntimeError, match="no U-Net"):
        _wrapper(pipeline_name=None, freeu=True)
    w = _wrapper(pipeline_name=None)
    with pytest.raises(RuntimeError, match="no U-Net"):
        w.enable_freeu()
    w.disable_freeu()
