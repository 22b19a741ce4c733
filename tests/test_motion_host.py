"""Motion modules, CPU only: the position table, the placement of the 21 temporal transformers, the strict loader on synthetic v1 / v2
state dicts, the U-Net's and the wrapper's refusals (none reaches the GPU), the plain-linear beta schedule, and the C entry point's
declaration, export and argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from adaface_dev_amd import _lib
from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper
from adaface_dev_amd.adaface.arc2face_models import clip_text_config
from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
from adaface_dev_amd.ldm.modules.motion_module import MotionModule, TemporalTransformer, motion_placement, sinusoidal_pe
from motion_util import direct_pe, motion_unet_cfg, prefix_channels, synth_motion_sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sd_v2():
    return synth_motion_sd(motion_unet_cfg(), with_mid=True, max_len=32)


@pytest.fixture(scope="module")
def sd_v1():
    return synth_motion_sd(motion_unet_cfg(), with_mid=False, max_len=24)


# ---------------------------------------------------------------------------------------------------------------- position table
@pytest.mark.parametrize("max_len,C", [(24, 64), (32, 320), (32, 6)])
def test_position_table_is_the_written_formula(max_len, C):
    pe = sinusoidal_pe(max_len, C)
    assert pe.shape == (1, max_len, C) and pe.dtype == torch.float32
    assert float((pe.double() - direct_pe(max_len, C)).abs().max()) <= 2.0 ** -23        # one fp32 rounding of values in [-1, 1]
    assert torch.equal(TemporalTransformer(64, 8, 24).transformer_blocks[0].attention_blocks[1].pos_encoder.pe, sinusoidal_pe(24, 64))


# ---------------------------------------------------------------------------------------------------------------- placement
def test_placement_of_all_21_prefixes():
    want = {
        "down_blocks.0.motion_modules.0": ("input", 1), "down_blocks.0.motion_modules.1": ("input", 2),
        "down_blocks.1.motion_modules.0": ("input", 4), "down_blocks.1.motion_modules.1": ("input", 5),
        "down_blocks.2.motion_modules.0": ("input", 7), "down_blocks.2.motion_modules.1": ("input", 8),
        "down_blocks.3.motion_modules.0": ("input", 10), "down_blocks.3.motion_modules.1": ("input", 11),
        "mid_block.motion_modules.0": ("middle", 1),
        "up_blocks.0.motion_modules.0": ("output", 0), "up_blocks.0.motion_modules.1": ("output", 1), "up_blocks.0.motion_modules.2": ("output", 2),
        "up_blocks.1.motion_modules.0": ("output", 3), "up_blocks.1.motion_modules.1": ("output", 4), "up_blocks.1.motion_modules.2": ("output", 5),
        "up_blocks.2.motion_modules.0": ("output", 6), "up_blocks.2.motion_modules.1": ("output", 7), "up_blocks.2.motion_modules.2": ("output", 8),
        "up_blocks.3.motion_modules.0": ("output", 9), "up_blocks.3.motion_modules.1": ("output", 10), "up_blocks.3.motion_modules.2": ("output", 11),
    }
    assert motion_placement(True) == want and len(want) == 21
    v1 = dict(want)
    del v1["mid_block.motion_modules.0"]
    assert motion_placement(False) == v1


def test_placed_widths_match_the_unet(sd_v2):
    """Every transformer sits where the U-Net has its width, and the Upsample of output blocks 2, 5 and 8 comes behind it."""
    cfg = motion_unet_cfg()
    unet = UNetModel(**cfg)
    mm = MotionModule(sd_v2)
    unet.set_motion(mm, 8)
    chans = prefix_channels(cfg)
    for prefix, (where, n) in motion_placement(True).items():
        block = unet.middle_block if where == "middle" else (unet.input_blocks if where == "input" else unet.output_blocks)[n]
        assert mm.at(where, n).channels == chans[prefix] == block[0].out_channels
    assert mm.at("input", 0) is None and mm.at("input", 3) is None and mm.at("middle", 0) is None
    assert not any(k.startswith("_motion") or "temporal" in k for k in unet.state_dict())
    unet.set_motion(None)
    assert unet._motion is None


# ---------------------------------------------------------------------------------------------------------------- loader
def test_v1_and_v2_state_dicts_load(sd_v1, sd_v2, tmp_path):
    m1, m2 = MotionModule(sd_v1), MotionModule(sd_v2)
    assert (m1.max_len, m1.with_mid, len(m1.transformers)) == (24, False, 20)
    assert (m2.max_len, m2.with_mid, len(m2.transformers)) == (32, True, 21)
    assert m1.at("middle", 1) is None and m2.at("middle", 1) is not None
    tt = m2.at("output", 5)
    key = "up_blocks.1.motion_modules.2.temporal_transformer.transformer_blocks.0.attention_blocks.1.to_k.weight"
    assert torch.equal(tt.transformer_blocks[0].attention_blocks[1].to_k.weight, sd_v2[key])
    assert torch.equal(tt.transformer_blocks[0].ff.net[2].bias,
                       sd_v2["up_blocks.1.motion_modules.2.temporal_transformer.transformer_blocks.0.ff.net.2.bias"])
    assert tt.norm.eps == 1e-6 and tt.norm.num_groups == 32 and tt.transformer_blocks[0].norms[0].eps == 1e-5
    assert not any(p.requires_grad for p in m2.parameters())
    # a file, with the optional 'module.' prefix and a 'state_dict' wrapper
    path = tmp_path / "mm.ckpt"
    torch.save({"state_dict": {"module." + k: v for k, v in sd_v1.items()}}, path)
    m3 = MotionModule(str(path))
    assert all(torch.equal(a, b) for a, b in zip(m1.state_dict().values(), m3.state_dict().values()))
    # a file without the position tables: they are computed
    m4 = MotionModule({k: v for k, v in sd_v2.items() if not k.endswith("pos_encoder.pe")})
    assert m4.max_len == 32
    assert torch.equal(m4.at("input", 1).transformer_blocks[0].attention_blocks[0].pos_encoder.pe, sinusoidal_pe(32, 64))


def test_loading_is_strict(sd_v2):
    gone = "down_blocks.2.motion_modules.1.temporal_transformer.transformer_blocks.0.ff_norm.bias"
    with pytest.raises(ValueError, match="missing.*" + re.escape(gone)):
        MotionModule({k: v for k, v in sd_v2.items() if k != gone})
    whole = "up_blocks.3.motion_modules.2.temporal_transformer."
    with pytest.raises(ValueError, match="missing.*" + re.escape(whole + "norm.weight")):
        MotionModule({k: v for k, v in sd_v2.items() if not k.startswith(whole)})
    for extra in ("up_blocks.0.motion_modules.0.temporal_transformer.transformer_blocks.0.attention_blocks.2.to_q.weight",
                  "down_blocks.0.motion_modules.2.temporal_transformer.norm.weight", "conv_in.weight"):
        with pytest.raises(ValueError, match="unexpected.*" + re.escape(extra)):
            MotionModule(dict(sd_v2, **{extra: torch.zeros(64, 64)}))
    bad = "mid_block.motion_modules.0.temporal_transformer.proj_out.weight"
    with pytest.raises(ValueError, match="wrong shape.*" + re.escape(bad)):
        MotionModule(dict(sd_v2, **{bad: torch.zeros(256, 128)}))
    pe = "down_blocks.0.motion_modules.0.temporal_transformer.transformer_blocks.0.attention_blocks.0.pos_encoder.pe"
    with pytest.raises(ValueError, match="pos_encoder.pe"):
        MotionModule(dict(sd_v2, **{pe: torch.zeros(1, 24, 64)}))
    with pytest.raises(ValueError, match="pos_encoder.pe"):
        MotionModule({k: (torch.zeros(1, 48, v.shape[2]) if k.endswith("pos_encoder.pe") else v) for k, v in sd_v2.items()})


# ---------------------------------------------------------------------------------------------------------------- U-Net
def test_unet_refusals_with_a_motion_module_set(sd_v1, sd_v2):
    cfg = motion_unet_cfg()
    unet = UNetModel(**cfg)
    assert unet._motion is None
    mm = MotionModule(sd_v1)
    for nf in (0, 25, -1):
        with pytest.raises(ValueError, match="num_frames"):
            unet.set_motion(mm, nf)
    wide = UNetModel(**dict(cfg, model_channels=128))
    with pytest.raises(ValueError, match="channels"):
        wide.set_motion(mm, 8)
    assert unet._motion is None and wide._motion is None
    unet.set_motion(mm, 24)
    x = torch.zeros(24, 8, 8, 8)
    t = torch.zeros(24, dtype=torch.long)
    ctx = torch.zeros(24, 77, 128)
    with pytest.raises(NotImplementedError, match="hip_train"):
        unet.hip_train(x, t, ctx)
    with pytest.raises(NotImplementedError, match="trunk"):
        unet.hip_trunk(x, None, ctx, None, 3)
    with pytest.raises(NotImplementedError, match="trunk"):
        unet.hip_tail((x, []), t, ctx, ())
    with pytest.raises(NotImplementedError, match="score-rewrite"):
        unet(torch.zeros(24, 4, 8, 8), t, ctx, extra_info={"normalize_cross_attn": True})
    with pytest.raises(NotImplementedError, match="training"):
        unet(torch.zeros(24, 4, 8, 8, requires_grad=True), t, ctx, extra_info={})
    unet.set_motion(None)


# ---------------------------------------------------------------------------------------------------------------- wrapper
def _wrapper(pipeline_name="text2img", **kw):
    cc = clip_text_config(hidden_size=64, num_attention_heads=1, num_hidden_layers=1, intermediate_size=128)
    return AdaFaceWrapper(pipeline_name=pipeline_name, clip_config=cc, unet_config=dict(motion_unet_cfg(), context_dim=64), device="cpu", **kw)


def _spy_apply(w):
    calls = []

    def spy(*a, **k):
        calls.append(a)
        raise AssertionError("the U-Net was reached")

    w.ldm.apply_model = spy
    return calls


def test_wrapper_video_refusals_need_no_gpu(sd_v1):
    from PIL import Image
    from test_inpaint_host import _vae
    pe = torch.zeros(1, 77, 64)
    noise = torch.zeros(2 * 8, 4, 8, 8)
    w = _wrapper()
    calls = _spy_apply(w)
    run = lambda wr=w, n=noise, **kw: wr(n, None, prompt_embeds=(pe, pe), out_image_count=2, **kw)
    with pytest.raises(ValueError, match="no motion module is loaded"):
        run(num_frames=8)
    assert w.load_motion_module(sd_v1) is w.motion_module and w.motion_module.max_len == 24
    assert not any("temporal_transformer" in k for k in w.state_dict())
    with pytest.raises(ValueError, match="hires_size"):
        run(num_frames=8, hires_size=(128, 128))
    for nf in (0, 25, -3, 2.0, True):
        with pytest.raises(ValueError, match="num_frames must be an integer from 1 to 24"):
            run(num_frames=nf)
    for n in (torch.zeros(15, 4, 8, 8), torch.zeros(2, 4, 8, 8), torch.zeros(16, 4, 8)):
        with pytest.raises(ValueError, match="out_image_count \\* num_frames = 16"):
            run(n=n, num_frames=8)
    assert calls == [] and w.ldm.model.diffusion_model._motion is None
    w.unload_motion_module()
    with pytest.raises(ValueError, match="no motion module is loaded"):
        run(num_frames=8)
    img = Image.fromarray(np.zeros((64, 64, 3), dtype=np.uint8))
    for name in ("img2img", "inpaint"):
        wi = _wrapper(name, vae=_vae(), motion_module_path=sd_v1)
        calls_i = _spy_apply(wi)
        with pytest.raises(ValueError, match="only pipeline_name='text2img' generates video"):
            wi(img, None, prompt_embeds=(pe, pe), out_image_count=2, num_frames=8,
               **({"mask_image": img.convert("L")} if name == "inpaint" else {}))
        assert calls_i == []
    # a module of another width is refused at load time
    from motion_util import synth_motion_sd as synth
    with pytest.raises(ValueError, match="channels"):
        w.load_motion_module(synth(dict(motion_unet_cfg(), model_channels=128), with_mid=False, max_len=24))
    assert w.motion_module is None


def test_num_frames_none_is_the_image_call_even_with_a_module_loaded(sd_v1):
    """One sampler.sample call with the arguments forward has always passed; the U-Net's motion state is never set."""
    w = _wrapper(num_inference_steps=10, motion_module_path=sd_v1)
    log = []

    class Rec:
        def sample(self, S, batch_size, shape, **kw):
            log.append((S, batch_size, tuple(shape), kw["conditioning"][0].shape[0], w.ldm.model.diffusion_model._motion))
            return kw["x_T"] + 1.0, {}

    w._sampler = lambda: Rec()
    pe = torch.zeros(1, 77, 64)
    noise = torch.zeros(6, 4, 8, 8)
    out = w(noise, None, prompt_embeds=(pe, pe), out_image_count=6)
    assert log == [(10, 6, (4, 8, 8), 6, None)] and torch.equal(out, noise + 1.0)
    # with num_frames: the batch is videos x frames, the module is on the U-Net during the call only, the latents come back video-major
    log.clear()
    out = w(noise, None, prompt_embeds=(pe, pe), out_image_count=2, num_frames=3)
    assert [e[:4] for e in log] == [(10, 6, (4, 8, 8), 6)] and log[0][4] == (w.motion_module, 3)
    assert w.ldm.model.diffusion_model._motion is None and torch.equal(out, noise + 1.0)


# ---------------------------------------------------------------------------------------------------------------- schedule
def test_beta_schedule_passes_through():
    w = _wrapper(beta_schedule="sqrt_linear")
    want = np.cumprod(1.0 - np.linspace(0.00085, 0.012, 1000, dtype=np.float64))
    assert np.array_equal(w.ldm.alphas_cumprod.numpy(), want.astype(np.float32))
    scaled = np.cumprod(1.0 - np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2)
    assert np.allclose(_wrapper().ldm.alphas_cumprod.numpy(), scaled, rtol=1e-6, atol=0)          # the default is unchanged
    with pytest.raises(ValueError, match="beta_schedule"):
        _wrapper(beta_schedule="sqrt_linear", ldm=w.ldm)


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_entry_point_is_declared_exported_and_checks_its_arguments():
    with open(os.path.join(ROOT, "include", "adaface_hip.h")) as f:
        header = f.read()
    assert ("int af_temporal_attention(const void* qkv, int ld, void* out, int B, int F, int HW, int heads, int d, float scale, void* stream);"
            in header)
    assert "af_temporal_attention" in _lib.EXPORTS
    L = _lib.lib()
    assert hasattr(L, "af_temporal_attention")
    buf = ctypes.create_string_buffer(4096 + 16)                       # host memory: every call below must be refused before any launch
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    call = lambda q=p, ld=96, o=p, B=1, F=4, HW=2, heads=2, d=16: L.af_temporal_attention(q, ld, o, B, F, HW, heads, d, 0.25, None)
    for kw in (dict(F=0), dict(F=33), dict(d=12), dict(d=0), dict(d=168, ld=1008), dict(ld=88), dict(ld=100), dict(q=None), dict(o=None),
               dict(q=p + 8), dict(o=p + 2), dict(B=0), dict(HW=0), dict(heads=0), dict(B=1 << 15, HW=1 << 15, F=2),
               dict(B=4096, HW=4096, F=2, heads=2, d=32, ld=192)):
        assert call(**kw) == _lib.AF_E_BADARG, kw
        assert b"af_temporal_attention" in L.af_last_error()
