"""High-resolution text2img host logic, CPU only (INTEGRATION.md "High-resolution text2img"): the ABI entry of the latent-upscale
kernel, the wrapper's refusals before any GPU work, the sequence of calls forward makes with and without hires_size, the step counts of
the second pass, and a transcription of the kernel's coordinate and weight rules against torch's F.interpolate on the CPU."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from adaface_dev_amd import TINY_UNET_CONFIG, _lib, rng
from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper
from adaface_dev_amd.adaface.arc2face_models import clip_text_config
from adaface_dev_amd.ldm.models.diffusion.ddim import DDIMSampler
from adaface_dev_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
from adaface_dev_amd.ldm.models.diffusion.lcm import LCMSampler
from test_inpaint_host import _Model, _vae
from test_lcm_host import restated_targets, synth_lora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (P, h, w, H, W) of the kernel tests (tests/test_hip_hires.py runs the same list on the GPU): ratios 2 and 3; ratios 1 and 1.5; odd
# sizes with one axis up and one down (W % 4 != 0); a single source pixel (every tap clamps); identity; the workload's ratio
SHAPES = [(8, 8, 8, 16, 24), (8, 16, 16, 16, 24), (4, 5, 7, 13, 9), (4, 1, 1, 4, 4), (3, 12, 8, 12, 8), (4, 64, 64, 128, 96)]
MODES = ("bilinear", "bicubic")


def test_header_and_exports_carry_the_kernel():
    with open(os.path.join(ROOT, "include", "adaface_hip.h")) as f:
        header = f.read()
    assert "int af_latent_resize_q_sample(const void* x, const void* noise, void* out, int P, int h, int w, int H, int W, int mode," in header
    assert "af_latent_resize_q_sample" in _lib.EXPORTS


# ---------------------------------------------------------------------------------------------------------------- wrapper
def _wrapper(pipeline_name="text2img", **kw):
    cc = clip_text_config(hidden_size=64, num_attention_heads=1, num_hidden_layers=1, intermediate_size=128)
    return AdaFaceWrapper(pipeline_name=pipeline_name, clip_config=cc, unet_config=dict(TINY_UNET_CONFIG), device="cpu", **kw)


def _spy_apply(w):
    calls = []

    def spy(*a, **k):
        calls.append(a)
        raise AssertionError("the U-Net was reached")

    w.ldm.apply_model = spy
    return calls


def _img():
    from PIL import Image
    return Image.fromarray(np.random.default_rng(0).integers(0, 256, (64, 64, 3), dtype=np.uint8))


def test_wrapper_hires_refuses_before_any_gpu_work():
    """Every refusal is a ValueError raised on the host, with zero U-Net calls (on the CPU the U-Net would fail anyway)."""
    pe = torch.zeros(1, 77, 64)
    noise = torch.zeros(1, 4, 8, 8)
    w = _wrapper(num_inference_steps=50)
    calls = _spy_apply(w)
    run = lambda **kw: w(noise, None, prompt_embeds=(pe, pe), out_image_count=1, **kw)
    for size in ((100, 128), (128, 100), (96, 128)):                       # a side that is no multiple of 64
        with pytest.raises(ValueError, match="multiples of 64"):
            run(hires_size=size)
    for size in ((0, 128), (128, 0), (1088, 128), (128, 1088), (-64, 64)):   # a side outside 64 .. 1024
        with pytest.raises(ValueError, match="64 to 1024"):
            run(hires_size=size)
    with pytest.raises(ValueError, match="hires_size"):
        run(hires_size=128)
    for name in ("nearest", "lanczos", None):
        with pytest.raises(ValueError, match="hires_upscaler"):
            run(hires_size=(128, 128), hires_upscaler=name)
    for strength in (0.0, 1.5, -0.2):
        with pytest.raises(ValueError, match=r"strength must be in \(0, 1\]"):
            run(hires_size=(128, 128), hires_strength=strength)
    with pytest.raises(ValueError, match="leaves no denoising step"):
        run(hires_size=(128, 128), hires_strength=0.01)
    with pytest.raises(ValueError, match="leaves no denoising step"):
        run(hires_size=(128, 128), hires_strength=0.3, hires_steps=3)
    for steps in (0, -5, 1001, 2.5):
        with pytest.raises(ValueError, match="hires_steps"):
            run(hires_size=(128, 128), hires_steps=steps)
    assert calls == []
    # LCM takes 1 .. 50 steps
    lsd = synth_lora(w.ldm.model.diffusion_model, restated_targets(), 4, seed=8)
    wl = _wrapper(use_lcm=True, lcm_lora_path=lsd, num_inference_steps=4)
    calls = _spy_apply(wl)
    with pytest.raises(ValueError, match="LCM takes 1 to 50"):
        wl(noise, None, prompt_embeds=(pe, pe), out_image_count=1, hires_size=(128, 128), hires_steps=51)
    assert calls == []
    # the other pipelines do not run two passes
    for name in ("img2img", "inpaint"):
        wi = _wrapper(name, vae=_vae())
        calls = _spy_apply(wi)
        with pytest.raises(ValueError, match="only pipeline_name='text2img'"):
            wi(_img(), None, prompt_embeds=(pe, pe), out_image_count=1, hires_size=(128, 128),
               **({"mask_image": _img().convert("L")} if name == "inpaint" else {}))
        assert calls == []


class _Recorder(DDIMSampler):
    """DDIMSampler's schedule and img2img_steps with the two sampling entry points replaced by recorders."""

    def __init__(self, model, log):
        super().__init__(model)
        self.log = log

    def sample(self, S, batch_size, shape, **kw):
        self.log.append(("sample", S, batch_size, tuple(shape), kw))
        return kw["x_T"] + 1.0, {}

    def sample_img2img(self, S, strength, batch_size, x_t, conditioning, **kw):
        self.log.append(("sample_img2img", S, strength, batch_size, x_t, conditioning, kw))
        return x_t * 2.0, {}


def _recorded_wrapper(steps=10):
    w = _wrapper(num_inference_steps=steps)
    log = []
    w._sampler = lambda: _Recorder(w.ldm, log)
    w.ldm.hires_latents = lambda *a: log.append(("hires_latents",) + a) or torch.full((2, 4, 16, 24), 3.0)
    return w, log


def test_forward_without_hires_size_is_unchanged():
    """hires_size=None: one sampler.sample call with the arguments forward has always passed, nothing else, its latents returned; the
    other three keywords are not looked at."""
    pe, ne = torch.zeros(1, 77, 64), torch.ones(1, 77, 64)
    noise = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(0))
    g = torch.Generator().manual_seed(1)
    for extra in ({}, dict(hires_strength=7.0, hires_steps=-1, hires_upscaler="nearest")):
        w, log = _recorded_wrapper()
        out = w(noise, "p", prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=2, generator=g, **extra)
        assert len(log) == 1
        name, S, B, shape, kw = log[0]
        assert (name, S, B, shape) == ("sample", 10, 2, (4, 8, 8))
        assert sorted(kw) == ["conditioning", "generator", "guidance_scale", "unconditional_conditioning", "verbose", "x_T"]
        assert torch.equal(kw["x_T"], noise) and kw["generator"] is g and kw["guidance_scale"] == 4.0 and kw["verbose"] is False
        assert torch.equal(kw["conditioning"][0], pe.repeat(2, 1, 1)) and torch.equal(kw["unconditional_conditioning"][0], ne.repeat(2, 1, 1))
        assert torch.equal(out, noise + 1.0)


@pytest.mark.parametrize("hires_steps,strength,n2_t", [(None, 0.7, (7, 601)), (4, 0.5, (2, 251))])
def test_forward_with_hires_size_chains_the_two_passes(hires_steps, strength, n2_t):
    """sample -> hires_latents(first-pass latents, (H/8, W/8), t_first, generator, upscaler) -> sample_img2img(S2, strength, ..., x_t)
    with the same conditioning, guidance value and generator; without a vae the second pass's latents come back."""
    pe, ne = torch.zeros(1, 77, 64), torch.ones(1, 77, 64)
    noise = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(0))
    g = torch.Generator().manual_seed(1)
    w, log = _recorded_wrapper()
    kw = {} if hires_steps is None else {"hires_steps": hires_steps}
    out = w(noise, "p", prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=2, generator=g, hires_size=(192, 128),
            hires_strength=strength, hires_upscaler="bicubic", **kw)
    S2 = hires_steps or 10
    assert DDIMSampler(w.ldm).img2img_steps(S2, strength) == n2_t
    assert [e[0] for e in log] == ["sample", "hires_latents", "sample_img2img"]
    first, hl, second = log
    assert first[1:4] == (10, 2, (4, 8, 8))
    assert torch.equal(hl[1], noise + 1.0) and tuple(hl[2]) == (16, 24) and hl[3] == n2_t[1] and hl[4] is g and hl[5] == "bicubic"
    _, S, st, B, x_t, cond, skw = second
    assert (S, st, B) == (S2, strength, 2) and torch.equal(x_t, torch.full((2, 4, 16, 24), 3.0))
    assert cond is first[4]["conditioning"] and skw["unconditional_conditioning"] is first[4]["unconditional_conditioning"]
    assert skw["guidance_scale"] == 4.0 and skw["generator"] is g
    assert torch.equal(out, torch.full((2, 4, 16, 24), 6.0))


def test_second_pass_step_counts():
    """img2img_steps(S2, hires_strength) of each sampler: the last n2 steps of the S2-step schedule."""
    m = _Model()
    assert DDIMSampler(m).img2img_steps(50, 0.7) == (35, 681)
    assert DDIMSampler(m).img2img_steps(4, 0.5) == (2, 251)
    assert DPMSolverSampler(m).img2img_steps(20, 0.7) == (14, 699)
    assert DPMSolverSampler(m).img2img_steps(8, 0.5) == (4, 500)
    assert LCMSampler(m).img2img_steps(4, 0.5) == (2, 499)
    assert LCMSampler(m).img2img_steps(8, 0.7) == (5, 639)
    for cls, S, strength in ((DDIMSampler, 50, 0.7), (DPMSolverSampler, 20, 0.7), (LCMSampler, 4, 0.5), (DDIMSampler, 30, 1.0)):
        s = cls(m)
        n, t = s.img2img_steps(S, strength)
        assert n == min(int(S * strength), S) and t == int(s.timesteps(S)[-n])


# ---------------------------------------------------------------------------------------------------------------- the written contract
def _taps(mode, n_in, n_out):
    """Per output index of one axis, the (source index, weight) pairs of the kernel contract (INTEGRATION.md "High-resolution
    text2img", af_latent_resize_q_sample), in Python floats."""
    scale = n_in / n_out
    out = []
    for dst in range(n_out):
        src = scale * (dst + 0.5) - 0.5
        if mode == "bilinear":
            src = max(src, 0.0)
            i0 = int(src)
            lam = src - i0
            out.append([(i0, 1.0 - lam), (min(i0 + 1, n_in - 1), lam)])
        else:
            i = math.floor(src)
            t = src - i
            A = -0.75
            c1 = lambda x: ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
            c2 = lambda x: ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A
            wts = [c2(t + 1.0), c1(t), c1(1.0 - t), c2((1.0 - t) + 1.0)]
            out.append([(min(max(i - 1 + k, 0), n_in - 1), wts[k]) for k in range(4)])
    return out


def restated_resize(x, H, W, mode):
    """x fp64 [P, h, w] -> [P, H, W]: the taps of _taps along each row first, then across the rows."""
    P, h, w = x.shape
    rows = np.zeros((P, h, W))
    for X, taps in enumerate(_taps(mode, w, W)):
        for i, wt in taps:
            rows[:, :, X] += wt * x[:, :, i]
    out = np.zeros((P, H, W))
    for Y, taps in enumerate(_taps(mode, h, H)):
        for i, wt in taps:
            out[:, Y, :] += wt * rows[:, i, :]
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_written_contract_is_torch_interpolate(shape, mode):
    """The coordinate and weight rules as written, evaluated in fp64, against F.interpolate(align_corners=False) in fp64 on the CPU.
    Both sum a handful of products of magnitude <= 1.6 max|x| per axis: 1e-13 max|x| is hundreds of fp64 roundings."""
    P, h, w, H, W = shape
    x = rng.synth_input("hires.x", (1, P, h, w), seed=h * 100 + W).double()
    ref = F.interpolate(x, size=(H, W), mode=mode, align_corners=False)[0].numpy()
    got = restated_resize(x[0].numpy(), H, W, mode)
    err = float(np.abs(got - ref).max())
    assert err <= 1e-13 * float(x.abs().max()), err
    if (h, w) == (H, W):
        assert np.array_equal(got, x[0].numpy())             # weights (1, 0) and (0, 1, 0, 0) at t = 0
