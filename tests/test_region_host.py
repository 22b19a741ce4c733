"""Regional prompts on the host: the launch plan with regions, the weight rule, the wrapper's refusals (each before any device work) and
``UNetModel.set_regions``' refusals.  Nothing here needs a GPU."""
import numpy as np
import pytest
import torch

from adaface_dev_amd import ops
from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper
from adaface_dev_amd.adaface.arc2face_models import clip_text_config
from adaface_dev_amd.ldm.modules import attention as A
from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
from motion_util import motion_unet_cfg


# ---------------------------------------------------------------------------------------------------------------- plan
def test_block_plan_with_regions():
    from test_block_plan_host import BLOCK, SWITCH_DEFAULTS
    saved = {k: getattr(A, k) for k in SWITCH_DEFAULTS}
    routes = set()
    try:
        for sw, (C, B, N, L), cap1, cap2, can_fold, _ in BLOCK:
            for k, v in {**SWITCH_DEFAULTS, **sw}.items():
                setattr(A, k, v)
            for want in (True, False):
                kw = dict(capture1=cap1, capture2=cap2, want_proj_out=want, can_fold_proj_out=can_fold)
                plain, off, on = (A.block_plan(C, B, N, L, 8, C, **kw), A.block_plan(C, B, N, L, 8, C, regions=False, **kw),
                                  A.block_plan(C, B, N, L, 8, C, regions=True, **kw))
                assert off == plain
                assert on.xattn == "split" and (on.ln12, on.ln3, on.ff) == (plain.ln12, plain.ln3, plain.ff), (sw, C, B, N, L)
                routes.add(plain.xattn)
                assert A.xattn_route(C, B, N, L, 8, C, not plain.ln12, cap2, chain=not cap1, regions=True) == "split"
                assert A.xattn_route(C, B, N, L, 8, C, not plain.ln12, cap2, chain=not cap1) == plain.xattn
    finally:
        for k, v in saved.items():
            setattr(A, k, v)
    assert {"fused", "chain", "split"} <= routes       # the grid reaches both one-launch routes the keyword excludes


def test_xattn_route_at_the_production_shapes():
    """The 64 x 64 level of an 8-row batch runs "fused" (and "chain" where the self-attention's to_out is offered); with regions it is "split";
    the same calls without the keyword are what they were."""
    assert A.xattn_route(320, 8, 4096, 77, 8, 320, True) == "fused"
    assert A.xattn_route(320, 8, 4096, 77, 8, 320, True, chain=True) == "chain"
    assert A.xattn_route(320, 8, 4096, 77, 8, 320, True, regions=True) == "split"
    assert A.xattn_route(320, 8, 4096, 77, 8, 320, True, chain=True, regions=True) == "split"
    assert A.xattn_route(320, 8, 4096, 77, 8, 320, True, regions=False) == "fused"


# ---------------------------------------------------------------------------------------------------------------- the weight rule
def rule_np(m, beta):
    """m float64 [R-1, N] in [0, 1] -> w [R, N]."""
    s = m.sum(0)
    return np.concatenate([(beta + (1 - beta) * (1 - np.minimum(1, s)))[None], (1 - beta) * m / np.maximum(1, s)], 0)


def test_weight_rule_sums_overlaps_and_beta():
    g = np.random.default_rng(5)
    m = g.random((3, 50))
    m[:, :10] = 0                       # no region: the base prompt alone
    m[0, 10:20], m[1, 10:20], m[2, 10:20] = 1, 0, 0      # one hard region
    m[:, 20:30] = 1                     # three regions overlap fully
    for beta in (0.0, 0.2, 1.0):
        w = rule_np(m, beta)
        assert np.allclose(w.sum(0), 1.0, atol=1e-12) and (w >= 0).all()
        assert np.array_equal(w[:, :10], np.array([[1.0], [0], [0], [0]]).repeat(10, 1))
        assert np.allclose(w[:, 10:20], np.array([[beta], [1 - beta], [0], [0]]))
        assert np.allclose(w[:, 20:30], np.array([[beta]] + [[(1 - beta) / 3]] * 3))
        assert (w[1:][m == 0] == 0).all()
    assert np.array_equal(rule_np(m, 1.0)[0], np.ones(50))
    assert ops.REGION_MAX == 8 and ops.region_level_sizes(512, 512) == [4096, 1024, 256, 64]


# ---------------------------------------------------------------------------------------------------------------- wrapper
CFG64 = dict(motion_unet_cfg(), context_dim=64)


def _wrapper(pipeline_name="text2img", **kw):
    cc = clip_text_config(hidden_size=64, num_attention_heads=1, num_hidden_layers=1, intermediate_size=128)
    return AdaFaceWrapper(pipeline_name=pipeline_name, clip_config=cc, unet_config=CFG64, device="cpu", **kw)


def test_wrapper_refusals_need_no_gpu(monkeypatch):
    from PIL import Image
    pe = torch.zeros(1, 77, 64)
    emb = (pe, pe)
    w = _wrapper()
    reached = []
    w.ldm.apply_model = lambda *a, **k: reached.append("unet") or (_ for _ in ()).throw(AssertionError("the U-Net was reached"))
    monkeypatch.setattr(ops, "region_weights", lambda *a, **k: reached.append("weights") or (_ for _ in ()).throw(AssertionError("device work")))
    monkeypatch.setattr(w, "encode_prompt", lambda *a, **k: reached.append("encode") or (_ for _ in ()).throw(AssertionError("the text encoder was reached")))
    m = np.zeros((64, 64), dtype=np.uint8)
    m[:, :32] = 255
    run = lambda **kw: w(torch.zeros(2, 4, 8, 8), None, prompt_embeds=emb, out_image_count=2, **kw)
    with pytest.raises(ValueError, match="2 region masks but 1 region prompts"):
        run(region_masks=[m, m], region_prompts=["a"])
    with pytest.raises(ValueError, match="1 region masks but 2 region prompts"):
        run(region_masks=[m], region_prompt_embeds=[emb, emb])
    with pytest.raises(ValueError, match="at most 7 regions"):
        run(region_masks=[m] * 8, region_prompts=["a"] * 8)
    for bad in (np.zeros((64, 32), dtype=np.uint8), Image.fromarray(np.zeros((128, 128), dtype=np.uint8)), torch.zeros(32, 64, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="the region masks must be the image's size, 64 x 64 pixels"):
            run(region_masks=[bad], region_prompts=["a"])
    with pytest.raises(ValueError, match="the region masks differ in size"):
        run(region_masks=[m, np.zeros((64, 32), dtype=np.uint8)], region_prompts=["a", "b"])
    with pytest.raises(ValueError, match="uint8"):
        run(region_masks=[m.astype(np.float32)], region_prompts=["a"])
    for beta in (-0.1, 1.5, float("nan"), None, "0.2", True):
        with pytest.raises(ValueError, match=r"region_base_weight must be in \[0, 1\]"):
            run(region_masks=[m], region_prompts=["a"], region_base_weight=beta)
    with pytest.raises(ValueError, match="exactly one of region_prompts"):
        run(region_masks=[m], region_prompts=["a"], region_prompt_embeds=[emb])
    with pytest.raises(ValueError, match="exactly one of region_prompts"):
        run(region_masks=[m])
    with pytest.raises(ValueError, match="without region_masks"):
        run(region_prompts=["a"])
    with pytest.raises(ValueError, match="region_prompts must be strings"):
        run(region_masks=[m], region_prompts=[3])
    with pytest.raises(ValueError, match="one encode_prompt result"):
        run(region_masks=[m], region_prompt_embeds=[pe])
    with pytest.raises(ValueError, match="not built with hires_size"):
        run(region_masks=[m], region_prompts=["a"], hires_size=(128, 128))
    with pytest.raises(ValueError, match="multiples of 64"):
        w(torch.zeros(2, 4, 8, 12), None, prompt_embeds=emb, out_image_count=2, region_masks=[np.zeros((64, 96), dtype=np.uint8)], region_prompts=["a"])
    # video: the wrapper's own video checks come first without a motion module, so check the regions' refusal directly as well
    with pytest.raises(ValueError, match="not built with num_frames"):
        w._check_regions([m], ["a"], None, 0.2, 4, None, None)
    with pytest.raises(ValueError, match="not built with crop_padding"):
        w._check_regions([m], ["a"], None, 0.2, None, None, 0.5)
    assert reached == [] and w.ldm.model.diffusion_model._regions is None


def test_wrapper_sets_regions_around_the_sampling_call_only(monkeypatch):
    """forward drives a recording sampler: the regions are on the U-Net during the call, with set 0 the base prompt, and gone afterwards --
    also when the sampler raises."""
    w = _wrapper(num_inference_steps=2)
    unet = w.ldm.model.diffusion_model
    got = []
    unet.set_regions = lambda c, u=None, lv=None: unet.__dict__.__setitem__("_regions", None if c is None else {"c": c, "u": u, "lv": lv})
    monkeypatch.setattr(ops, "region_weights", lambda masks, beta: (None, [("level", tuple(masks.shape), beta)]))

    class Rec:
        boom = False

        def sample(self, S, batch_size, shape, callback=None, **kw):
            got.append(unet._regions)
            if self.boom:
                raise RuntimeError("the sampler failed")
            return kw["x_T"], {}

    rec = Rec()
    w._sampler = lambda: rec
    base, neg, a, b = (torch.full((1, 77, 64), v) for v in (1.0, -1.0, 2.0, 3.0))
    m = np.zeros((64, 64), dtype=np.uint8)
    kw = dict(prompt_embeds=(base, neg), out_image_count=2, region_masks=[m, m], region_prompt_embeds=[(a, neg), (b, neg)], region_base_weight=0.3)
    w(torch.zeros(2, 4, 8, 8), None, **kw)
    st = got[0]
    assert unet._regions is None and st is not None
    assert st["c"].dtype == torch.float16 and tuple(st["c"].shape) == (2, 3, 77, 64) and tuple(st["u"].shape) == (2, 77, 64)
    assert [float(st["c"][1, r, 0, 0]) for r in range(3)] == [1.0, 2.0, 3.0] and float(st["u"][1, 0, 0]) == -1.0
    assert st["lv"] == [("level", (2, 64, 64), 0.3)]
    rec.boom = True
    with pytest.raises(RuntimeError, match="the sampler failed"):
        w(torch.zeros(2, 4, 8, 8), None, **kw)
    assert got[1] is not None and unet._regions is None
    rec.boom = False
    w(torch.zeros(2, 4, 8, 8), None, prompt_embeds=(base, neg), out_image_count=2)       # without the arguments: no regions
    assert got[2] is None
    # region_prompts: strings, encoded through encode_prompt (so with the subject currently set), one call per region
    asked = []
    monkeypatch.setattr(w, "encode_prompt", lambda t, n=None, **k: asked.append(t) or (torch.full((1, 77, 64), float(len(asked)) + 4.0), neg, None, None))
    w(torch.zeros(2, 4, 8, 8), None, prompt_embeds=(base, neg), out_image_count=2, region_masks=[m, m], region_prompts=["left", "right"])
    assert asked == ["left", "right"] and [float(got[3]["c"][0, r, 0, 0]) for r in range(3)] == [1.0, 5.0, 6.0]
    assert got[3]["lv"] == [("level", (2, 64, 64), 0.2)] and unet._regions is None


# ---------------------------------------------------------------------------------------------------------------- U-Net state
def test_set_regions_refusals():
    cfg = motion_unet_cfg()
    unet = UNetModel(**cfg)
    cc = unet._cross_attn_layers()[0].to_k.in_features
    c = torch.zeros(1, 2, 77, cc, dtype=torch.float16)
    u = torch.zeros(1, 77, cc, dtype=torch.float16)
    lv = [torch.zeros(2, 64), torch.zeros(2, 16)]
    for bad in (c.float(), c[0], torch.zeros(1, 9, 77, cc, dtype=torch.float16), torch.zeros(1, 2, 81, cc, dtype=torch.float16),
                torch.zeros(1, 2, 77, cc + 8, dtype=torch.float16), "x"):
        with pytest.raises(ValueError, match="contexts must be fp16"):
            unet.set_regions(bad, u, lv)
    for bad in (u.float(), u.repeat(2, 1, 1), u[:, :70], None):
        with pytest.raises(ValueError, match="uncond_context must be fp16"):
            unet.set_regions(c, bad, lv)
    for bad in (None, [], torch.zeros(2, 64)):
        with pytest.raises(ValueError, match="weights must be the levels' fp32 tensors"):
            unet.set_regions(c, u, bad)
    for bad in ([torch.zeros(3, 64)], [torch.zeros(2, 64, dtype=torch.float16)], [torch.zeros(64)]):
        with pytest.raises(ValueError, match="every level's weights must be fp32"):
            unet.set_regions(c, u, bad)
    with pytest.raises(ValueError, match="the same token count"):
        unet.set_regions(c, u, [torch.zeros(2, 64), torch.zeros(2, 64)])
    assert unet._regions is None
    unet.__dict__["_regions"] = {"rows": 1, "R": 2, "L": 77}          # as set_regions leaves it: every other walk refuses by name
    for call in (lambda: unet.hip_train(None, None, None), lambda: unet.hip_trunk(None, None, None, None, 3), lambda: unet.hip_tail(None, None, None, (), 3),
                 lambda: unet.hip(None, None, None, None, (22,)), lambda: unet.set_motion(object(), 4)):
        with pytest.raises(NotImplementedError, match="not built with regional prompts"):
            call()
    with pytest.raises(ValueError, match="neither the regions' rows"):
        unet._place_regions(3)
    layer = unet._cross_attn_layers()[0]
    layer._region_pre = (None, None, 0, 0, {}, 2)
    with pytest.raises(NotImplementedError, match="hip_train is not built with regional prompts"):
        layer.hip_train(None, 1, 1, context=torch.zeros(1, 1, cc))
    with pytest.raises(NotImplementedError, match="hip_bwd is not built with regional prompts"):
        layer.hip_bwd(None, None)
    layer.save_cross_attn_vars = True
    with pytest.raises(NotImplementedError, match="the capture path"):
        layer.hip(None, 1, 1, context=torch.zeros(1, 1, cc))
    unet.set_regions(None)
    assert unet._regions is None
    unet.__dict__["_motion"] = (object(), 4)
    with pytest.raises(NotImplementedError, match="set_regions is not built for video"):
        unet.set_regions(c, u, lv)
