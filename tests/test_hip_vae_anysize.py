"""The VAE at any image size on a real MI355X (`pytest -m gpu`): the fused single-head attention kernel ``af_vae_attention`` (head dim 128 /
512, any token count % 8 == 0) against fp32 torch, the VAE's ``decode`` / ``encode`` at sizes its three-launch attention refuses against
the CPU oracle, and the wrapper's three pipelines end to end at such sizes.

Bounds: 2e-3 rel-L2 for the kernel (``test_hip_kernels.TOL``: fp16 in, fp32 inside, one fp16 rounding out) and 1e-2 for the whole network
(``test_hip_vae.py``'s bound)."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from test_hip_kernels import TOL, rnd
from test_vae_oracle import VAE_SMALL, _probes

pytestmark = pytest.mark.gpu

VAE_TOL = 1e-2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _qkv(B, N, C, seed=1):
    """q (pre-scaled by C^-0.5, as _q_scaled_pack folds it), k, v: fp16 [B*N, C] on the CPU."""
    return rnd((B * N, C), seed, C ** -0.5), rnd((B * N, C), seed + 1), rnd((B * N, C), seed + 2)


def _ref_rows(q, k, v, B, N, rows=None):
    """fp32 softmax(q k^T) v of the fp16 inputs, per image; ``rows``: query indices (within an image) to compute, default all."""
    out = []
    for b in range(B):
        qb, kb, vb = (t[b * N:(b + 1) * N].float() for t in (q, k, v))
        if rows is not None:
            qb = qb[rows]
        o = torch.empty(qb.shape[0], vb.shape[1])
        for i in range(0, qb.shape[0], 1024):
            o[i:i + 1024] = torch.softmax(qb[i:i + 1024] @ kb.t(), dim=1) @ vb
        out.append(o)
    return torch.stack(out)


@pytest.mark.parametrize("B,N,C", [(1, 3136, 512), (2, 6144, 512), (1, 4096, 512), (3, 200, 512), (1, 8, 512), (1, 16384, 512),
                                   (2, 256, 128), (1, 6144, 128)])
def test_vae_attention_vs_fp32_torch(dev, B, N, C):
    """All rows; at N = 16384 the first and last 64 query rows plus a seeded sample (576 rows in all) against all keys."""
    from adaface_dev_amd import ops
    q, k, v = _qkv(B, N, C)
    o = ops.vae_attention(q.to(dev), k.to(dev), v.to(dev), B=B, N=N, C=C)
    assert o.shape == (B * N, C) and o.dtype == torch.float16
    o = o.float().cpu().reshape(B, N, C)
    assert bool(torch.isfinite(o).all())
    rows = None
    if N >= 16384:
        mid = torch.randperm(N - 128, generator=torch.Generator().manual_seed(7))[:448] + 64
        rows = torch.cat([torch.arange(64), mid.sort().values, torch.arange(N - 64, N)])
        o = o[:, rows]
    e = rel_l2(o.numpy(), _ref_rows(q, k, v, B, N, rows).numpy())
    print(f"af_vae_attention B={B} N={N} C={C}: rel-L2 vs fp32 torch = {e:.3e}")
    assert e < TOL


@pytest.mark.parametrize("N", [6144, 200])
def test_vae_attention_rows_are_convex_combinations(dev, N):
    """With V constant per channel the output is that constant (softmax rows sum to 1), whole key tiles and a key tail."""
    from adaface_dev_amd import ops
    B, C = 2, 512
    q, k, _ = _qkv(B, N, C, seed=11)
    const = rnd((C,), 13)
    v = const[None, :].expand(B * N, C).contiguous()
    o = ops.vae_attention(q.to(dev), k.to(dev), v.to(dev), B=B, N=N, C=C)
    err = (o.float().cpu() - const.float()[None, :]).abs().max().item()
    assert err < 4e-3 * const.float().abs().max().item() + 1e-3, (N, err)


def test_vae_attention_online_softmax_rescale_branch(dev):
    """The softmax reference must move late and start low (after test_attention_online_softmax_rescale_branch, same fp32 reference and
    bound): a spiked key in the LAST key tile, one in a MIDDLE tile, and a strongly NEGATIVE first tile for one query, all far beyond
    the kernel's 2^8 lazy margin."""
    from adaface_dev_amd import ops
    B, N, C = 1, 6144, 512
    q, k, v = rnd((N, C), 1, C ** -0.5), rnd((N, C), 2, 0.3), rnd((N, C), 3)
    sc = float(C) ** 0.5
    k[N - 3] = (q[5].float() * sc * 4).half()           # score ~ 4 |q5|^2 sqrt(C) ~ 90 against query 5 in the final tile
    k[3000] = (q[40].float() * sc * 4).half()           # query 40 (the block's second 32-query group) in a middle tile
    k[:32] = -(q[70].float() * sc * 2).half()           # query 70 starts from a strongly negative first tile
    o = ops.vae_attention(q.to(dev), k.to(dev), v.to(dev), B=B, N=N, C=C).float().cpu()
    assert bool(torch.isfinite(o).all())
    ref = _ref_rows(q, k, v, B, N)[0]
    assert rel_l2(o.numpy(), ref.numpy()) < TOL
    for i in (5, 40, 70):
        assert rel_l2(o[i].numpy(), ref[i].numpy()) < 5 * TOL, i       # the spiked rows one by one: a lost rescale is O(1) there


@pytest.mark.parametrize("B,N,C", [(2, 200, 512), (1, 3136, 512), (2, 72, 128)])
def test_vae_attention_poisoned_padding(dev, B, N, C):
    """q / k / v / o live inside larger NaN-filled buffers (wider rows and rows beyond B*N): the rows are those of the plain call, nothing
    beyond B*N rows or C columns of o is written, and nothing outside the logical inputs reaches o."""
    from adaface_dev_amd import _lib, ops
    q, k, v = _qkv(B, N, C, seed=21)
    want = ops.vae_attention(q.to(dev), k.to(dev), v.to(dev), B=B, N=N, C=C)
    ld, extra = C + 64, 96
    bufs = []
    for t in (q, k, v):
        buf = torch.full((B * N + extra, ld), float("nan"), dtype=torch.float16, device=dev)
        buf[:B * N, :C] = t.to(dev)
        bufs.append(buf)
    got = ops.vae_attention(bufs[0][:B * N, :C], bufs[1][:B * N, :C], bufs[2][:B * N, :C], B=B, N=N, C=C)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    # the C ABI directly, with a padded V^T (keys N .. ldv - 1 NaN) and a padded, NaN-filled output
    ldv = N + 40
    vt = torch.full((B, C, ldv), float("nan"), dtype=torch.float16, device=dev)
    vt[:, :, :N] = v.to(dev).reshape(B, N, C).permute(0, 2, 1)
    obuf = torch.full((B * N + extra, ld), float("nan"), dtype=torch.float16, device=dev)
    rc = _lib.lib().af_vae_attention(bufs[0].data_ptr(), bufs[1].data_ptr(), vt.data_ptr(), obuf.data_ptr(), B, N, C, ld, ld, ldv, ld,
                                     ops._stream())
    _lib.check(rc, "af_vae_attention")
    torch.cuda.synchronize()
    assert torch.equal(obuf[:B * N, :C], want)
    assert bool(torch.isnan(obuf[B * N:]).all()) and bool(torch.isnan(obuf[:, C:]).all())


def test_vae_attention_flash_and_gemm_paths_agree_with_fp32(dev, monkeypatch):
    """N = 4096, C = 512, the one size both forms take: the attention layer under AF_VAE_FLASH=1 and with the switch off each stay within
    2e-3 of fp32 torch on the same fp16 q / k / v (bit equality is neither expected nor asserted)."""
    from adaface_dev_amd import ops
    from adaface_dev_amd.ldm.modules.diffusionmodules import model as M
    B, N, C = 1, 4096, 512
    q, k, v = _qkv(B, N, C, seed=31)
    ref = _ref_rows(q, k, v, B, N)[0].numpy()
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    assert M.vae_attention_path(N, C) == "gemm" and M.vae_attention_path(N, C, flash_env=True) == "flash"
    fused = ops.vae_attention(qd, kd, vd, B=B, N=N, C=C)
    vt = ops.transpose_tokens(vd, B, N, C, C)
    p = ops.softmax_rows(ops.gemm(qd, ops.PackedWeight(kd, None, N, C, C, 1, C)))
    three = ops.gemm(p, ops.PackedWeight(vt[0], None, C, N, N, 1, N))
    e_f, e_g = rel_l2(fused.float().cpu().numpy(), ref), rel_l2(three.float().cpu().numpy(), ref)
    print(f"N=4096 C=512 rel-L2 vs fp32: af_vae_attention {e_f:.3e}, GEMM + af_softmax_rows + GEMM {e_g:.3e}")
    assert e_f < TOL and e_g < TOL
    # and through the layer: the switch picks the kernel, the two layer outputs agree to the same bound
    from adaface_dev_amd import rng
    blk = M.AttnBlock(C)
    with torch.no_grad():
        for n, prm in blk.named_parameters():
            prm.copy_(rng.synth_tensor("attn." + n, prm.shape, seed=33))
    blk = blk.to(dev).eval()
    x = rnd((1, 64, 64, C), 34).to(dev)
    calls = []
    real = ops.vae_attention
    monkeypatch.setattr(ops, "vae_attention", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    monkeypatch.delenv("AF_VAE_FLASH", raising=False)
    y_gemm = blk.hip(x)
    assert not calls
    monkeypatch.setenv("AF_VAE_FLASH", "1")
    y_flash = blk.hip(x)
    assert len(calls) == 1
    assert rel_l2(y_flash.float().cpu().numpy(), y_gemm.float().cpu().numpy()) < TOL


# ------------------------------------------------------------------------------------------------------------------ the VAE
def _small_ae(dev, seed=92):
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.modules.diffusionmodules.model import AutoencoderKL
    ae = AutoencoderKL(dict(VAE_SMALL, double_z=True))
    with torch.no_grad():
        for n, p in ae.named_parameters():
            p.copy_(rng.synth_tensor(n, p.shape, seed=seed))
    sd = {k: v.detach().float().clone() for k, v in ae.state_dict().items()}
    return ae.to(dev).eval(), sd


def _small_kw():
    return dict(num_resolutions=len(VAE_SMALL["ch_mult"]), num_res_blocks=VAE_SMALL["num_res_blocks"])


@pytest.mark.parametrize("shape", [(2, 4, 56, 56), (1, 4, 96, 64), (1, 4, 128, 128), (2, 4, 24, 40)])
def test_vae_decode_and_encode_any_size_reduced_width_vs_oracle(dev, shape):
    """decode of a latent and encode of the matching image at token counts the three-launch attention refuses (3136, 6144, 16384, 960)."""
    from adaface_dev_amd import rng
    from oracle import vae_oracle as VO
    ae, sd = _small_ae(dev)
    up = 2 ** (len(VAE_SMALL["ch_mult"]) - 1)
    B, _, h, w = shape
    z = rng.synth_input(f"vae.any.z.{h}x{w}", shape, seed=94)
    with torch.no_grad():
        img = ae.decode(z.to(dev)).cpu()
        ref = VO.decode(sd, z, **_small_kw())
    assert img.shape == (B, 3, h * up, w * up)
    e = rel_l2(img.numpy(), ref.numpy())
    print(f"decode {shape} (reduced width) rel-L2 vs oracle: {e:.3e}")
    assert e < VAE_TOL
    x = rng.synth_input(f"vae.any.img.{h}x{w}", (B, 3, h * up, w * up), seed=95)
    with torch.no_grad():
        mean, logvar = ae.encode(x.to(dev))
        rm, rl = VO.encode(sd, x)
    assert mean.shape == (B, 4, h, w)
    em, el = rel_l2(mean.cpu().numpy(), rm.numpy()), rel_l2(logvar.cpu().numpy(), rl.numpy())
    print(f"encode {tuple(x.shape)} (reduced width) rel-L2 vs oracle: mean {em:.3e}, logvar {el:.3e}")
    assert em < VAE_TOL and el < VAE_TOL


def test_vae_sd15_width_decode_96x64_and_encode_448_vs_oracle(dev):
    """The SD-1.5 VAE (synthetic weights) where the fused kernel runs at C = 512: decode of one [1, 4, 96, 64] latent (6144 tokens, a
    768 x 512 image) and encode of one 448 x 448 image (3136 tokens), each against the CPU oracle in full (no crop: the fp32 reference is
    ~2 TFLOP of convolutions, tens of seconds on 16 threads)."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.modules.diffusionmodules.model import AutoencoderKL
    from oracle import vae_oracle as VO
    ae = AutoencoderKL()
    with torch.no_grad():
        for n, p in ae.named_parameters():
            p.copy_(rng.synth_tensor(n, p.shape, seed=90))
    sd = {k: v.detach().float().clone() for k, v in ae.state_dict().items()}
    ae = ae.to(dev).eval()
    z = rng.synth_input("vae.any.z.full", (1, 4, 96, 64), seed=96)
    with torch.no_grad():
        img = ae.decode(z.to(dev)).cpu()
        ref = VO.decode(sd, z)
    assert img.shape == (1, 3, 768, 512)
    e = rel_l2(img.numpy(), ref.numpy())
    print(f"decode [1, 4, 96, 64] (SD-1.5 width) rel-L2 vs oracle: {e:.3e}")
    assert e < VAE_TOL
    assert np.allclose(_probes(img), _probes(ref), rtol=5e-2, atol=2e-2)
    x = rng.synth_input("vae.any.img.full", (1, 3, 448, 448), seed=97)
    with torch.no_grad():
        mean, logvar = ae.encode(x.to(dev))
        rm, rl = VO.encode(sd, x)
    assert mean.shape == (1, 4, 56, 56)
    em, el = rel_l2(mean.cpu().numpy(), rm.numpy()), rel_l2(logvar.cpu().numpy(), rl.numpy())
    print(f"encode 448 x 448 (SD-1.5 width) rel-L2 vs oracle: mean {em:.3e}, logvar {el:.3e}")
    assert em < VAE_TOL and el < VAE_TOL


# ------------------------------------------------------------------------------------------------------------------ the wrapper
def _wrapper(dev, pipeline_name, scheduler="ddim"):
    """The reduced-width stand-ins of test_hip_img2img / test_hip_inpaint: small CLIP, 64-channel U-Net, VAE_SMALL, synthetic weights."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper
    from adaface_dev_amd.adaface.arc2face_models import clip_text_config
    from adaface_dev_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    from test_hip_img2img import _unet_cfg
    cc = clip_text_config(hidden_size=128, num_attention_heads=2, num_hidden_layers=3, intermediate_size=512)
    ld = LatentDiffusion(_unet_cfg())
    ae = ld.instantiate_first_stage(dict(VAE_SMALL, double_z=True))
    with torch.no_grad():
        for n, p in ae.named_parameters():
            p.copy_(rng.synth_tensor(n, p.shape, seed=92))
    w = AdaFaceWrapper(pipeline_name=pipeline_name, clip_config=cc, ldm=ld, vae=ae, device=dev, num_inference_steps=5,
                       default_scheduler_name=scheduler)
    rng.load_synth_weights(w.ldm.model.diffusion_model, seed=63)
    pe = rng.synth_input("inp.pe", (1, 77, 128), seed=85).to(dev)
    ne = rng.synth_input("inp.ne", (1, 77, 128), seed=86).to(dev)
    return w.to(dev), ae, pe, ne


def _finite_images(out, n, size):
    assert len(out) == n and all(im.size == size for im in out)
    a = np.stack([np.asarray(im) for im in out])
    assert a.dtype == np.uint8 and a.std() > 0           # a NaN image would have become a constant one


def test_wrapper_img2img_448x320_end_to_end(dev):
    """A 448 x 320 photo (56 x 40 latent: 2240 tokens, not a multiple of 128) through img2img under DPM-Solver++."""
    from test_hip_img2img import _pil
    w, ae, pe, ne = _wrapper(dev, "img2img", "dpm++")
    lat = []
    orig = ae.decode
    ae.decode = lambda zz: (lat.append(zz), orig(zz))[1]
    try:
        out = w(_pil(448, 320, seed=5), None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=2, ref_img_strength=0.8,
                generator=torch.Generator().manual_seed(7))
    finally:
        del ae.decode
    _finite_images(out, 2, (448, 320))
    assert lat[0].shape == (2, 4, 40, 56) and bool(torch.isfinite(lat[0]).all())


def test_wrapper_inpaint_768x512_end_to_end(dev):
    """A 768 x 512 photo with a mask (96 x 64 latent, 6144 tokens): finite, and where the latent mask is 0 the latent handed to decode is
    z / 0.18215 exactly, as test_wrapper_inpaint_vs_oracle_reduced_width asserts at 128 x 128."""
    from adaface_dev_amd.adaface.adaface_wrapper import img2img_images_u8, inpaint_masks
    from test_hip_img2img import _pil
    from test_hip_inpaint import _mask_pil
    w, ae, pe, ne = _wrapper(dev, "inpaint")
    img, mask = _pil(768, 512, seed=4), _mask_pil(768, 512)
    lat = []
    orig = ae.decode
    ae.decode = lambda zz: (lat.append(zz), orig(zz))[1]
    try:
        out = w(img, None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=2, ref_img_strength=0.8,
                generator=torch.Generator().manual_seed(7), mask_image=mask)
    finally:
        del ae.decode
    _finite_images(out, 2, (768, 512))
    assert lat[0].shape == (2, 4, 64, 96) and bool(torch.isfinite(lat[0]).all())
    _, z, _ = w.ldm.inpaint_latents(img2img_images_u8(img, 2).to(dev), 2, 601, generator=torch.Generator().manual_seed(7),
                                    first_stage_model=ae)
    m = inpaint_masks(mask, 2, (768, 512))
    assert 0 < float(m.mean()) < 1
    keep = (m == 0).expand(2, 4, 64, 96)
    assert torch.equal(lat[0].cpu()[keep], (z[[0, 0]] / 0.18215).cpu()[keep])


def test_wrapper_text2img_96x64_noise_end_to_end(dev):
    """text2img from [2, 4, 96, 64] noise: two 512 x 768 (W x H) images; before the fused kernel this failed in _to_pil after the last step."""
    w, ae, pe, ne = _wrapper(dev, "text2img")
    noise = torch.randn(2, 4, 96, 64, generator=torch.Generator().manual_seed(9))
    lat = []
    orig = ae.decode
    ae.decode = lambda zz: (lat.append(zz), orig(zz))[1]
    try:
        out = w(noise, None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=2)
    finally:
        del ae.decode
    _finite_images(out, 2, (512, 768))
    assert lat[0].shape == (2, 4, 96, 64) and bool(torch.isfinite(lat[0]).all())
