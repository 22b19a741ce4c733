"""Regional prompts through the modules on a real MI355X (`pytest -m gpu`): one ``CrossAttention.hip`` layer with regions placed, the U-Net
with ``set_regions`` (the small configuration of the other module tests), the launch plan of a full-width block, and the wrapper under the
three samplers and with an IP-Adapter.

Tolerances are measured in the test from code that is not under test: a plain layer's (the plain U-Net's) own fp16 error against the fp32
torch composition (the CPU oracle) at that shape, times two -- the regional core rounds where the plain core rounds (P once, o once), so
two results of that error each may differ by their sum."""
import numpy as np
import pytest
import torch

from ip_adapter_util import ip_inputs, synth_ip_sd
from motion_util import motion_unet_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- one layer
def _layer_fp32(sd, x, ctx, heads):
    """CrossAttention.forward as a plain fp32 torch composition on the CPU: x [B, N, C], ctx [B, L, cc] -> [B, N, C]."""
    B, N, _ = x.shape
    q, k, v = x @ sd["to_q.weight"].t(), ctx @ sd["to_k.weight"].t(), ctx @ sd["to_v.weight"].t()
    d = q.shape[-1] // heads
    split = lambda t: t.reshape(B, -1, heads, d).permute(0, 2, 1, 3)
    p = torch.softmax(split(q) @ split(k).transpose(-1, -2) * d ** -0.5, dim=-1)
    o = (p @ split(v)).permute(0, 2, 1, 3).reshape(B, N, heads * d)
    return o @ sd["to_out.0.weight"].t() + sd["to_out.0.bias"]


def test_layer_with_two_hard_half_image_regions_matches_the_plain_layer_per_half(dev):
    """A 16 x 16-token layer (C = 128, 8 heads of 16) with three context sets: a base set of weight 0, A on the left half, B on the right half.
    The left half's rows are the plain layer's under A, the right half's under B."""
    from adaface_dev_amd import ops, rng
    from adaface_dev_amd.ldm.modules import attention as A
    C, cc, heads, d, side, L, B = 128, 64, 8, 16, 16, 77, 2
    N = side * side
    layer = A.CrossAttention(C, cc, heads=heads, dim_head=d)
    rng.load_synth_weights(layer, seed=91)
    sd = {k: v.detach().clone().float() for k, v in layer.state_dict().items()}
    layer = layer.to(dev).eval()
    x = rng.synth_input("rg.x", (B, N, C), seed=92).half()
    ctxs = [rng.synth_input(f"rg.ctx{r}", (B, L, cc), seed=93 + r).half() for r in range(3)]          # base, A, B
    left = (torch.arange(N) % side < side // 2)
    w = torch.zeros((B, 3, N))
    w[:, 1, left] = 1.0
    w[:, 2, ~left] = 1.0
    x2d = x.reshape(B * N, C).to(dev)

    def plain(ctx):
        with torch.no_grad():
            y = layer.hip(x2d, B, N, context=ctx.to(dev))
        torch.cuda.synchronize()
        return y.cpu().float().reshape(B, N, C)

    ya, yb = plain(ctxs[1]), plain(ctxs[2])
    e16 = max(float((ya - _layer_fp32(sd, x.float(), ctxs[1].float(), heads)).abs().max()),
              float((yb - _layer_fp32(sd, x.float(), ctxs[2].float(), heads)).abs().max()))
    tol = 2 * e16
    # the sets as batch items b R + r of one projection, as UNetModel.set_regions lays them out
    stacked = torch.stack(ctxs, 1).reshape(B * 3 * L, cc).to(dev).contiguous()
    k, vt = ops.gemm(stacked, layer._packed_kv(), rows_per_batch=L, split_col=C)
    layer._region_pre = (k, vt, k.stride(0), vt.stride(0), {N: w.reshape(B * 3, N).to(dev)}, 3)
    try:
        with torch.no_grad():
            y = layer.hip(x2d, B, N, context=ctxs[0].to(dev))
        torch.cuda.synchronize()
    finally:
        layer._region_pre = None
    y = y.cpu().float().reshape(B, N, C)
    el, er = float((y[:, left] - ya[:, left]).abs().max()), float((y[:, ~left] - yb[:, ~left]).abs().max())
    cross = float((y[:, left] - yb[:, left]).abs().max())
    print(f"layer with two half-image regions: left vs plain(A) {el:.3e}, right vs plain(B) {er:.3e}, tolerance 2 x e16 = {tol:.3e}; "
          f"left vs plain(B) {cross:.3e}")
    assert el <= tol and er <= tol
    assert cross > 2 * tol                           # the two contexts do tell the halves apart
    assert torch.equal(plain(ctxs[1]), ya)           # and the layer is the plain layer again


# ---------------------------------------------------------------------------------------------------------------- U-Net
@pytest.fixture(scope="module")
def net(dev):
    """(unet on the device, its CPU state dict)."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    unet = UNetModel(**motion_unet_cfg())
    rng.load_synth_weights(unet, seed=63)
    sd = {k: v.detach().clone() for k, v in unet.state_dict().items()}
    return unet.to(dev).eval(), sd


def _eps(unet, dev, x, t, ctx):
    with torch.no_grad():
        e = unet(x.to(dev), t.to(dev), ctx.to(dev), extra_info={})
    torch.cuda.synchronize()
    return e.cpu()


def test_unet_one_white_region_with_the_base_context_is_the_plain_walk(dev, net):
    """rows = 1, batch 2 (cond, uncond), 64 x 64 pixels: one all-white region whose context is the base context splits the same attention into
    0.2 + 0.8 of itself; the uncond row runs its own context under w = (1, 0).  ``set_regions(None)`` restores the plain walk bit-exactly."""
    from adaface_dev_amd import ops, rng
    from oracle import unet_oracle as O
    unet, sd = net
    cfg = motion_unet_cfg()
    cc = cfg["context_dim"]
    x = rng.synth_input("rg.unet.x", (1, 4, 8, 8), seed=95).repeat(2, 1, 1, 1)
    t = torch.tensor([400, 400])
    pe, ne = rng.synth_input("rg.unet.pe", (1, 77, cc), seed=96), rng.synth_input("rg.unet.ne", (1, 77, cc), seed=97)
    ctx = torch.cat([pe, ne])
    before = _eps(unet, dev, x, t, ctx)
    e16 = float((before - O.unet_forward(sd, cfg, x, t, ctx, {})).abs().max())
    white = torch.full((1, 64, 64), 255, dtype=torch.uint8, device=dev)
    _, levels = ops.region_weights(white, 0.2)
    assert [tuple(l.shape) for l in levels] == [(2, 64), (2, 16), (2, 4), (2, 1)]
    pe16 = pe.to(dev).half()
    unet.set_regions(torch.stack([pe16, pe16], 1), ne.to(dev).half(), levels)
    try:
        assert all(b.attn2._region_pre is None for b in _blocks(unet))
        with_regions = _eps(unet, dev, x, t, ctx)
        assert all(b.attn2._region_pre is None for b in _blocks(unet))          # placed during the walk only
        cond_only = _eps(unet, dev, x[:1], t[:1], ctx[:1])
        with pytest.raises(ValueError, match="neither the regions' rows"):
            _eps(unet, dev, x.repeat(2, 1, 1, 1)[:3], t.repeat(2)[:3], ctx.repeat(2, 1, 1)[:3])
    finally:
        unet.set_regions(None)
    err = float((with_regions - before).abs().max())
    print(f"U-Net with one white region = the base context: max |eps - plain eps| {err:.3e}, tolerance 2 x e16 = {2 * e16:.3e}")
    assert err <= 2 * e16
    assert float((cond_only - before[:1]).abs().max()) <= 2 * e16
    assert torch.equal(_eps(unet, dev, x, t, ctx), before)


def _blocks(unet):
    from adaface_dev_amd.ldm.modules.attention import BasicTransformerBlock
    return [m for m in unet.modules() if isinstance(m, BasicTransformerBlock)]


def test_unet_regions_change_eps_where_they_lie(dev, net):
    """A region on the left half under another context moves the cond row's eps (the halves' mean changes are printed: attention is per
    token, the convolutions and GroupNorm spread it), while the uncond row, which never reads the region, stays within twice the plain walk's
    own fp16 error against the CPU oracle."""
    from adaface_dev_amd import ops, rng
    from oracle import unet_oracle as O
    unet, sd = net
    cfg = motion_unet_cfg()
    cc = cfg["context_dim"]
    x = rng.synth_input("rg.unet.x", (1, 4, 8, 8), seed=95).repeat(2, 1, 1, 1)
    t = torch.tensor([400, 400])
    pe, ne, other = (rng.synth_input(f"rg.unet.{n}", (1, 77, cc), seed=s) for n, s in (("pe", 96), ("ne", 97), ("other", 98)))
    ctx = torch.cat([pe, ne])
    before = _eps(unet, dev, x, t, ctx)
    e16 = float((before - O.unet_forward(sd, cfg, x, t, ctx, {})).abs().max())
    m = torch.zeros((1, 64, 64), dtype=torch.uint8, device=dev)
    m[:, :, :32] = 255
    unet.set_regions(torch.stack([pe, 3.0 * other], 1).to(dev).half(), ne.to(dev).half(), ops.region_weights(m, 0.0)[1])
    try:
        after = _eps(unet, dev, x, t, ctx)
    finally:
        unet.set_regions(None)
    dl, dr = float((after[0, :, :, :4] - before[0, :, :, :4]).abs().mean()), float((after[0, :, :, 4:] - before[0, :, :, 4:]).abs().mean())
    du = float((after[1] - before[1]).abs().max())
    moved = float((after[0] - before[0]).abs().max())
    print(f"a left-half region: mean |d eps| left {dl:.3e}, right {dr:.3e}, max {moved:.3e}; uncond row max |d eps| {du:.3e}, 2 x e16 = {2 * e16:.3e}")
    assert bool(torch.isfinite(after).all()) and moved > 4 * e16
    assert du <= 2 * e16                              # the uncond row's walk does not depend on the cond row's regions


# ---------------------------------------------------------------------------------------------------------------- full-width block
def test_full_width_block_routes_split_with_regions_and_back(dev):
    """One SpatialTransformer at C = 320, N = 4096, B = 2, context 768: plain, the block takes the one-launch routes; with regions placed its attn2
    runs split: the top half matches the plain block under A, the bottom half under B; without them again it is bitwise what it was."""
    from adaface_dev_amd import ops, rng
    from adaface_dev_amd.ldm.modules import attention as A
    C, B, H, ctx_dim, L = 320, 2, 64, 768, 77
    N = H * H
    st = A.SpatialTransformer(C, 8, 40, context_dim=ctx_dim)
    rng.load_synth_weights(st, seed=71)
    st = st.to(dev).eval()
    block = st.transformer_blocks[0]
    x = rng.synth_input("rg.blk.x", (B, C, H, H), seed=72)
    ca, cb = rng.synth_input("rg.blk.a", (B, L, ctx_dim), seed=73), rng.synth_input("rg.blk.b", (B, L, ctx_dim), seed=74)
    assert block.plan(C, B, N, ca).xattn in ("chain", "fused")

    def run(ctx):
        with torch.no_grad():
            y = st(x.to(dev), ctx.to(dev))
        torch.cuda.synchronize()
        return y.cpu()

    ya, yb = run(ca), run(cb)
    top = torch.arange(N) < N // 2
    w = torch.zeros((B, 2, N))
    w[:, 0, top] = 1.0
    w[:, 1, ~top] = 1.0
    stacked = torch.stack([ca, cb], 1).reshape(B * 2 * L, ctx_dim).to(dev).half().contiguous()
    k, vt = ops.gemm(stacked, block.attn2._packed_kv(), rows_per_batch=L, split_col=C)
    block.attn2._region_pre = (k, vt, k.stride(0), vt.stride(0), {N: w.reshape(B * 2, N).to(dev)}, 2)
    try:
        assert block.plan(C, B, N, ca).xattn == "split"
        y = run(ca)
    finally:
        block.attn2._region_pre = None
    assert block.plan(C, B, N, ca).xattn in ("chain", "fused")
    assert torch.equal(run(ca), ya)
    # the one-launch block and the split block round differently: the tolerance is their own difference on the plain layer, times two
    saved = A.FUSE_XATTN
    A.FUSE_XATTN = False
    try:
        e16 = float((run(ca) - ya).abs().max())
    finally:
        A.FUSE_XATTN = saved
    ht = H // 2
    et, eb = float((y[:, :, :ht] - ya[:, :, :ht]).abs().max()), float((y[:, :, ht:] - yb[:, :, ht:]).abs().max())
    cross = float((y[:, :, :ht] - yb[:, :, :ht]).abs().max())
    print(f"C = 320 block with top / bottom regions: top vs plain(A) {et:.3e}, bottom vs plain(B) {eb:.3e}, split-vs-one-launch difference {e16:.3e}; "
          f"top vs plain(B) {cross:.3e}")
    assert e16 > 0 and et <= 2 * e16 and eb <= 2 * e16 and cross > 4 * e16


# ---------------------------------------------------------------------------------------------------------------- wrapper
def _lcm_lora(unet):
    from test_lcm_host import restated_targets, synth_lora
    return synth_lora(unet, restated_targets(), 8, seed=31, alpha=4, scale=0.5)


def _wrapper(dev, scheduler, ip_adapter=None, steps=2):
    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper
    from adaface_dev_amd.adaface.arc2face_models import clip_text_config
    from adaface_dev_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    cc = clip_text_config(hidden_size=128, num_attention_heads=2, num_hidden_layers=3, intermediate_size=512)
    ld = LatentDiffusion(motion_unet_cfg())
    rng.load_synth_weights(ld.model.diffusion_model, seed=63)
    kw = dict(use_lcm=True, lcm_lora_path=_lcm_lora(ld.model.diffusion_model)) if scheduler == "lcm" else dict(default_scheduler_name=scheduler)
    w = AdaFaceWrapper(pipeline_name="text2img", clip_config=cc, ldm=ld, vae=None, device=dev, num_inference_steps=steps, ip_adapter=ip_adapter, **kw)
    return w.to(dev)


@pytest.mark.parametrize("scheduler,with_ip", [("ddim", False), ("dpm++", False), ("lcm", False), ("ddim", True)])
def test_wrapper_two_regions_at_64_pixels(dev, scheduler, with_ip):
    """2 rows, 2 steps, CFG, latents out (vae=None), two regions given as ``region_prompt_embeds`` (the several-subjects recipe): finite,
    bit-exact under one seed, different from the call without regions, and the regions are off the U-Net afterwards -- also when the
    sampler raises."""
    from adaface_dev_amd import rng
    B, g = 2, (1.5 if scheduler == "lcm" else 4.0)
    w = _wrapper(dev, scheduler, synth_ip_sd(motion_unet_cfg(), "faceid") if with_ip else None)
    unet = w.ldm.model.diffusion_model
    pe, ne, ea, eb = (rng.synth_input(f"rg.w.{n}", (1, 77, 128), seed=s).to(dev) for n, s in (("pe", 85), ("ne", 86), ("a", 88), ("b", 89)))
    noise = rng.synth_input("rg.w.noise", (B, 4, 8, 8), seed=87).to(dev)
    m1, m2 = np.zeros((64, 64), dtype=np.uint8), np.zeros((64, 64), dtype=np.uint8)
    m1[:, :40] = 255                              # the two overlap in columns 24 .. 39
    m2[:, 24:] = 255
    extra = dict(ip_adapter_face_id=ip_inputs("faceid", rows=B)[3], ip_adapter_scale=0.8) if with_ip else {}
    run = lambda **kw: w(noise, None, prompt_embeds=(pe, ne), guidance_scale=g, out_image_count=B, generator=torch.Generator().manual_seed(3),
                         **extra, **kw).cpu()
    regions = dict(region_masks=[m1, m2], region_prompt_embeds=[(3.0 * ea, ne), (3.0 * eb, ne)], region_base_weight=0.2)
    plain = run()
    out = run(**regions)
    torch.cuda.synchronize()
    assert out.shape == (B, 4, 8, 8) and bool(torch.isfinite(out).all())
    assert unet._regions is None and unet._ip is None
    assert torch.equal(run(**regions), out)
    moved = float((out - plain).abs().max())
    print(f"wrapper ({scheduler}, ip={with_ip}) with two regions: max |latents - plain latents| {moved:.3e}")
    assert moved > 1e-3
    assert torch.equal(run(), plain)
    sampler = w._sampler()
    seen = []

    def boom(*a, **k):
        seen.append(unet._regions is not None)
        raise RuntimeError("the sampler failed")

    sampler.sample = boom
    w._sampler = lambda: sampler
    with pytest.raises(RuntimeError, match="the sampler failed"):
        run(**regions)
    assert seen == [True] and unet._regions is None
