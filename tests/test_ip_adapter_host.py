"""IP-Adapter on the host: the key table, the strict loader, the launch plan with image tokens, the FaceID LoRA fuse, the wrapper's refusals
and the teeth of the CPU restatement the GPU tests trust (tests/ip_adapter_util.py).  Nothing here needs a GPU."""
import numpy as np
import pytest
import torch

from adaface_dev_amd import rng
from adaface_dev_amd.adaface import ip_adapter as IP
from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper
from adaface_dev_amd.adaface.arc2face_models import clip_text_config
from adaface_dev_amd.ldm.modules import attention as A
from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
from conftest import rel_l2
from ip_adapter_util import (FAULTS, V_GAIN, diffusers_cross_attn_order, fused_unet_sd, image_proj_ref, ip_inputs, synth_ip_sd, unet_forward_ip)
from motion_util import motion_unet_cfg
from oracle import unet_oracle as O

NET_TOL = 4e-3             # test_hip_ip_adapter.NET_TOL: a fault of the walk must move eps by more than ten times what the GPU test allows


@pytest.fixture(scope="module")
def cfg():
    return motion_unet_cfg()


# ---------------------------------------------------------------------------------------------------------------- key table
def test_key_table_is_diffusers_processor_order(cfg):
    order = diffusers_cross_attn_order(cfg)                       # {odd i: LDM path}, enumerated down, up, mid
    assert sorted(order) == list(range(1, 32, 2))
    layout = IP.cross_attn_layout(cfg)
    unet = UNetModel(**cfg)
    names = {id(m): n for n, m in unet.named_modules()}
    own = [names[id(m)] for m in unet._cross_attn_layers()]       # the j order of the U-Net itself
    assert own == [p + ".transformer_blocks.0.attn2" for p, _ in layout]
    assert [m.inner_dim for m in unet._cross_attn_layers()] == [c for _, c in layout]
    assert len(IP.KEY_INDEX) == 16 and [order[i] for i in IP.KEY_INDEX] == [p for p, _ in layout]
    assert IP.KEY_INDEX == tuple([2 * j + 1 for j in range(6)] + [31] + [2 * j - 1 for j in range(7, 16)])
    # the LoRA keys: every i in 0 .. 31 once per leaf, even i on attn1 of the layer whose attn2 is i + 1
    paths = IP._lora_paths(layout)
    assert sorted({int(k.split(".")[0]) for k in paths}) == list(range(32)) and len(paths) == 32 * 4
    for i, p in order.items():
        assert paths[f"{i}.to_k_lora"] == p + ".transformer_blocks.0.attn2.to_k"
        assert paths[f"{i - 1}.to_out_lora"] == p + ".transformer_blocks.0.attn1.to_out.0"


# ---------------------------------------------------------------------------------------------------------------- loader
@pytest.mark.parametrize("kind", IP.KINDS)
@pytest.mark.parametrize("nested", [True, False])
def test_loader_reads_both_spellings_and_kinds(cfg, kind, nested, tmp_path):
    sd = synth_ip_sd(cfg, kind, nested=nested)
    ad = IP.load_ip_adapter(sd, cfg)
    assert ad.kind == kind and ad.num_tokens == 4 and len(ad.to_k_ip) == len(ad.to_v_ip) == 16
    flat = IP._flatten(sd)
    for j, i in enumerate(IP.KEY_INDEX):
        assert torch.equal(ad.to_k_ip[j].weight, flat[f"ip_adapter.{i}.to_k_ip.weight"])
        assert torch.equal(ad.to_v_ip[j].weight, flat[f"ip_adapter.{i}.to_v_ip.weight"])
    assert torch.equal(ad.image_proj.norm.weight, flat["image_proj.norm.weight"])
    assert len(ad.lora) == (128 if kind == "faceid" else 0)
    path = tmp_path / ("a.bin" if nested else "a.safetensors")
    if nested:
        torch.save(sd, path)
    else:
        from safetensors.torch import save_file
        save_file({k: v.contiguous() for k, v in sd.items()}, str(path))
    ad2 = IP.load_ip_adapter(str(path), cfg)
    assert all(torch.equal(a, b) for a, b in zip(ad.state_dict().values(), ad2.state_dict().values()))


@pytest.mark.parametrize("kind", IP.KINDS)
def test_loader_is_strict_and_names_the_key(cfg, kind):
    flat = synth_ip_sd(cfg, kind, nested=False)
    sd = dict(flat)
    del sd["ip_adapter.31.to_v_ip.weight"]
    with pytest.raises(ValueError, match=r"missing \['ip_adapter\.31\.to_v_ip\.weight'\]"):
        IP.load_ip_adapter(sd, cfg)
    with pytest.raises(ValueError, match=r"unexpected \['ip_adapter\.33\.to_k_ip\.weight'\]"):
        IP.load_ip_adapter(dict(flat, **{"ip_adapter.33.to_k_ip.weight": torch.zeros(64, 128)}), cfg)
    with pytest.raises(ValueError, match=r"mis-shaped \['ip_adapter\.13\.to_k_ip\.weight: \(128, 128\), want \(256, 128\)'\]"):
        IP.load_ip_adapter(dict(flat, **{"ip_adapter.13.to_k_ip.weight": torch.zeros(128, 128)}), cfg)
    with pytest.raises(ValueError, match="exactly the dicts 'image_proj' and 'ip_adapter'"):
        IP.load_ip_adapter({"image_proj": {}, "ip_adapter": {}, "extra": {}}, cfg)


def test_loader_refuses_plus_kind_mismatch_and_sdxl_by_name(cfg):
    clip, face = synth_ip_sd(cfg, "clip", nested=False), synth_ip_sd(cfg, "faceid", nested=False)
    plus = {k: v for k, v in clip.items() if not k.startswith("image_proj.")}
    plus.update({"image_proj.latents": torch.zeros(1, 16, 768), "image_proj.layers.0.0.norm1.weight": torch.zeros(768)})
    with pytest.raises(ValueError, match="IP-Adapter Plus"):
        IP.load_ip_adapter(plus, cfg)
    mixed = {k: v for k, v in face.items() if not k.startswith("image_proj.")}
    mixed.update({k: v for k, v in clip.items() if k.startswith("image_proj.")})
    with pytest.raises(ValueError, match="kind mismatch: image_proj is of kind 'clip' but ip_adapter holds FaceID LoRA keys"):
        IP.load_ip_adapter(mixed, cfg)
    mixed = {k: v for k, v in clip.items() if not k.startswith("image_proj.")}
    mixed.update({k: v for k, v in face.items() if k.startswith("image_proj.")})
    with pytest.raises(ValueError, match="kind mismatch: image_proj is of kind 'faceid' but ip_adapter holds no FaceID LoRA keys"):
        IP.load_ip_adapter(mixed, cfg)
    xl = dict(clip, **{"ip_adapter.1.to_k_ip.weight": torch.zeros(640, 2048)})
    with pytest.raises(ValueError, match="SDXL IP-Adapter"):
        IP.load_ip_adapter(xl, cfg)
    with pytest.raises(ValueError, match="kind must be one of"):
        IP.IPAdapter(cfg, "plus")
    with pytest.raises(ValueError, match="cross-attention layers, the SD-1.5 key table 16"):
        IP.IPAdapter(dict(cfg, attention_resolutions=[4, 2]), "clip")


# ---------------------------------------------------------------------------------------------------------------- plan
def test_block_plan_with_image_tokens():
    from test_block_plan_host import BLOCK, SWITCH_DEFAULTS
    saved = {k: getattr(A, k) for k in SWITCH_DEFAULTS}
    one_launch = 0
    try:
        for sw, (C, B, N, L), cap1, cap2, can_fold, _ in BLOCK:
            for k, v in {**SWITCH_DEFAULTS, **sw}.items():
                setattr(A, k, v)
            for want in (True, False):
                kw = dict(capture1=cap1, capture2=cap2, want_proj_out=want, can_fold_proj_out=can_fold)
                plain, off, on = A.block_plan(C, B, N, L, 8, C, **kw), A.block_plan(C, B, N, L, 8, C, ip=False, **kw), A.block_plan(C, B, N, L, 8, C, ip=True, **kw)
                assert off == plain
                assert on.xattn == "split" and (on.ln12, on.ln3, on.ff) == (plain.ln12, plain.ln3, plain.ff), (sw, C, B, N, L)
                one_launch += plain.xattn != "split"
                assert A.xattn_route(C, B, N, L, 8, C, not plain.ln12, cap2, chain=not cap1, ip=True) == "split"
    finally:
        for k, v in saved.items():
            setattr(A, k, v)
    assert one_launch > 10            # the grid does reach the one-launch routes the keyword excludes


# ---------------------------------------------------------------------------------------------------------------- LoRA
def test_faceid_lora_fuse_and_unfuse_on_cpu_weights(cfg):
    ipsd = synth_ip_sd(cfg, "faceid")
    ad = IP.load_ip_adapter(ipsd, cfg)
    unet = UNetModel(**cfg)
    rng.load_synth_weights(unet, seed=63)
    before = {k: v.detach().clone() for k, v in unet.state_dict().items()}
    ad.fuse(unet, 0.75)
    with pytest.raises(RuntimeError, match="already fused"):
        ad.fuse(unet, 0.75)
    want = fused_unet_sd(before, ipsd, cfg, 0.75)
    after = unet.state_dict()
    changed = [k for k in before if not torch.equal(before[k], after[k])]
    assert sorted(changed) == sorted(p + ".weight" for p in ad.lora) and len(changed) == 128
    for k in changed:
        assert float((after[k].double() - want[k].double()).abs().max()) <= 1e-5 * float(want[k].abs().max()), k
    ad.unfuse()
    assert all(torch.equal(before[k], v) for k, v in unet.state_dict().items())
    ad.unfuse()                                                    # a second unfuse is a no-op
    unet._merge_saved = {"x": 1}                                   # sd_lora.check_no_live_merge holds for this fuse too
    with pytest.raises(RuntimeError, match="DoRA adapter merge is live"):
        ad.fuse(unet, 1.0)


# ---------------------------------------------------------------------------------------------------------------- wrapper
CFG64 = dict(motion_unet_cfg(), context_dim=64)


def _wrapper(pipeline_name="text2img", **kw):
    cc = clip_text_config(hidden_size=64, num_attention_heads=1, num_hidden_layers=1, intermediate_size=128)
    return AdaFaceWrapper(pipeline_name=pipeline_name, clip_config=cc, unet_config=CFG64, device="cpu", **kw)


def test_wrapper_refusals_need_no_gpu():
    from PIL import Image
    pe = torch.zeros(1, 77, 64)
    img = Image.fromarray(np.zeros((32, 32, 3), dtype=np.uint8))
    fid = torch.nn.functional.normalize(torch.ones(1, 512), dim=-1)
    w = _wrapper()
    calls = []
    w.ldm.apply_model = lambda *a, **k: calls.append(a) or (_ for _ in ()).throw(AssertionError("the U-Net was reached"))
    run = lambda wr=w, **kw: wr(torch.zeros(2, 4, 8, 8), None, prompt_embeds=(pe, pe), out_image_count=2, **kw)
    for kw in (dict(ip_adapter_image=img), dict(ip_adapter_face_id=fid)):
        with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
            run(**kw)
    with pytest.raises(ValueError, match="ip_image_encoder is given without ip_adapter"):
        _wrapper(ip_image_encoder=object())
    # kind "clip"
    before = {k: v.clone() for k, v in w.ldm.model.state_dict().items()}
    ad = w.load_ip_adapter(synth_ip_sd(CFG64, "clip"))
    assert ad is w.ip_adapter and ad.kind == "clip" and not any("to_k_ip" in k or "image_proj" in k for k in w.state_dict())
    tokens = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the image projection was reached"))
    ad.tokens = tokens
    with pytest.raises(ValueError, match="needs an image encoder"):
        run(ip_adapter_image=img)
    with pytest.raises(ValueError, match="ip_adapter_face_id is given but the loaded adapter is of kind 'clip'"):
        run(ip_adapter_face_id=fid)
    w.__dict__["ip_image_encoder"] = object()                      # never reached below
    with pytest.raises(ValueError, match=r"1 image \(shared\) or one per sampled row \(2\) expected, got 3"):
        run(ip_adapter_image=[img] * 3)
    with pytest.raises(ValueError, match="ip_adapter_image must be a PIL image"):
        run(ip_adapter_image=torch.zeros(32, 32, 3))
    for s in (float("nan"), float("inf"), -float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="ip_adapter_scale must be a finite number"):
            run(ip_adapter_image=img, ip_adapter_scale=s)
    for start, end in ((-0.1, 1.0), (0.0, 1.1), (0.5, 0.5), (0.7, 0.3), (None, 1.0), (0.0, "1")):
        with pytest.raises(ValueError, match="0 <= ip_guidance_start < ip_guidance_end <= 1"):
            run(ip_adapter_image=img, ip_guidance_start=start, ip_guidance_end=end)
    # kind "faceid": the LoRA lives in the U-Net's weights while loaded
    ad = w.load_ip_adapter(synth_ip_sd(CFG64, "faceid"))
    ad.tokens = tokens
    assert ad.kind == "faceid" and any(not torch.equal(before[k], v) for k, v in w.ldm.model.state_dict().items())
    with pytest.raises(ValueError, match="it takes ip_adapter_face_id, or ip_adapter_image with a face_id_extractor"):
        run(ip_adapter_image=img)
    with pytest.raises(ValueError, match="not both"):
        run(ip_adapter_image=img, ip_adapter_face_id=fid)
    with pytest.raises(ValueError, match=r"one per sampled row \(2\) expected, got 3"):
        run(ip_adapter_face_id=fid.repeat(3, 1))
    for bad in (torch.zeros(1, 256), torch.zeros(512), torch.zeros(1, 512, dtype=torch.int64), [0.0] * 512):
        with pytest.raises(ValueError, match="ip_adapter_face_id must be a floating-point tensor"):
            run(ip_adapter_face_id=bad)
    assert calls == [] and w.ldm.model.diffusion_model._ip is None
    w.unload_ip_adapter()
    assert w.ip_adapter is None and all(torch.equal(before[k], v) for k, v in w.ldm.model.state_dict().items())
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        run(ip_adapter_face_id=fid)
    # an adapter of another width is refused at load time
    with pytest.raises(ValueError, match="does not fit this U-Net"):
        w.load_ip_adapter(synth_ip_sd(dict(CFG64, model_channels=128), "clip"))
    assert w.ip_adapter is None


def test_wrapper_switches_the_adapter_by_the_window():
    """forward drives a recording sampler: the adapter is on the U-Net during the call only, with the tokens computed once, and the callback
    switches it by the guidance-window rule (state seen BEFORE each step)."""
    w = _wrapper(ip_adapter=synth_ip_sd(CFG64, "faceid"), num_inference_steps=4)
    unet = w.ldm.model.diffusion_model
    made = []
    w._ip_tokens = lambda what, value, rows: made.append((what, rows)) or (torch.zeros(rows, 4, 64, dtype=torch.float16),) * 2
    unet.set_ip_adapter = lambda ad, *a, **k: unet.__dict__.__setitem__("_ip", None if ad is None else {"active": True, "scale": a[2]})
    seen = []

    class Rec:
        def timesteps(self, S):
            return list(range(S))

        def sample(self, S, batch_size, shape, callback=None, **kw):
            for i in range(S):
                seen.append(unet._ip is not None and unet._ip["active"])
                if callback:
                    callback(i)
            return kw["x_T"], {}

    w._sampler = lambda: Rec()
    pe = torch.zeros(1, 77, 64)
    fid = torch.ones(1, 512)
    for (start, end), want in (((0.0, 1.0), [True] * 4), ((0.0, 0.5), [True, True, False, False]), ((0.25, 0.75), [False, True, True, False])):
        seen.clear()
        made.clear()
        w(torch.zeros(2, 4, 8, 8), None, prompt_embeds=(pe, pe), out_image_count=2, ip_adapter_face_id=fid, ip_adapter_scale=0.5, ip_guidance_start=start,
          ip_guidance_end=end)
        assert seen == want and unet._ip is None and made == [("ids", 2)]
    seen.clear()
    w(torch.zeros(2, 4, 8, 8), None, prompt_embeds=(pe, pe), out_image_count=2)          # without the arguments: the sampler is called as before
    assert seen == [False] * 4 and made == [("ids", 2)]


def test_unet_state_refusals(cfg):
    unet = UNetModel(**cfg)
    ad = IP.load_ip_adapter(synth_ip_sd(cfg, "clip"), cfg)
    tok = torch.zeros(1, 4, 128, dtype=torch.float16)
    with pytest.raises(ValueError, match="no IP-Adapter is set"):
        unet.set_ip_adapter_active(True)
    for bad in (tok.float(), torch.zeros(1, 4, 64, dtype=torch.float16), torch.zeros(1, 65, 128, dtype=torch.float16), None):
        with pytest.raises(ValueError, match="cond_tokens must be fp16"):
            unet.set_ip_adapter(ad, bad, tok)
    with pytest.raises(ValueError, match="uncond_tokens"):
        unet.set_ip_adapter(ad, tok, tok.repeat(2, 1, 1))
    with pytest.raises(ValueError, match="scale must be finite"):
        unet.set_ip_adapter(ad, tok, tok, float("nan"))
    with pytest.raises(ValueError, match="to_k_ip of layer 0 maps"):
        unet.set_ip_adapter(IP.IPAdapter(dict(cfg, model_channels=128), "clip"), tok, tok)
    assert unet._ip is None
    unet.__dict__["_ip"] = {"active": True}                        # as set_ip_adapter leaves it: every other walk refuses
    for call in (lambda: unet.hip_train(None, None, None), lambda: unet.hip_trunk(None, None, None, None, 3), lambda: unet.hip_tail(None, None, None, (), 3),
                 lambda: unet.hip(None, None, None, None, (22,))):
        with pytest.raises(NotImplementedError, match="not built with an IP-Adapter"):
            call()
    layer = unet._cross_attn_layers()[0]
    layer._ip_pre = (None, None, 1.0)
    with pytest.raises(NotImplementedError, match="hip_train is not built with an IP-Adapter"):
        layer.hip_train(None, 1, 1, context=torch.zeros(1, 1, 128))
    unet.set_ip_adapter(None)
    assert unet._ip is None


# ---------------------------------------------------------------------------------------------------------------- reference teeth
@pytest.mark.parametrize("kind", IP.KINDS)
def test_reference_teeth(cfg, kind):
    """The CPU walk the GPU tests trust: without tokens (or at scale 0) it IS unet_oracle.unet_forward; with the synthetic to_v_ip at V_GAIN the
    adapter moves eps by far more than the GPU tolerance on the inputs the GPU tests use, and so does each single fault of the walk."""
    unet = UNetModel(**cfg)
    rng.load_synth_weights(unet, seed=63)
    sd = {k: v.detach().clone() for k, v in unet.state_dict().items()}
    ipsd = synth_ip_sd(cfg, kind)
    x, t, ctx, e = ip_inputs(kind)
    with torch.no_grad():
        cond, uncond = image_proj_ref(ipsd, kind, e).float(), image_proj_ref(ipsd, kind, torch.zeros_like(e)).float()
        plain = O.unet_forward(sd, cfg, x, t, ctx, {})
        assert torch.equal(unet_forward_ip(sd, ipsd, cfg, x, t, ctx, cond, uncond, fault="no_ip"), plain)
        assert rel_l2(unet_forward_ip(sd, ipsd, cfg, x, t, ctx, cond, uncond, scale=0.0).numpy(), plain.numpy()) < 1e-6
        good = unet_forward_ip(sd, ipsd, cfg, x, t, ctx, cond, uncond, scale=1.0)
        moved = rel_l2(good.numpy(), plain.numpy())
        print(f"{kind}, v_gain {V_GAIN}: the adapter moves eps by {moved:.3e}")
        assert moved > 0.05
        assert rel_l2(unet_forward_ip(sd, ipsd, cfg, x, t, ctx, cond, uncond, scale=0.5).numpy(), good.numpy()) > 10 * NET_TOL
        for fault in FAULTS:
            c, u = (image_proj_ref(ipsd, kind, v, norm=False).float() for v in (e, torch.zeros_like(e))) if fault == "no_norm" else (cond, uncond)
            d = rel_l2(unet_forward_ip(sd, ipsd, cfg, x, t, ctx, c, u, scale=1.0, fault=fault).numpy(), good.numpy())
            print(f"{kind}, fault {fault}: eps moves by {d:.3e}")
            assert d > 10 * NET_TOL, (fault, d)
