"""Face IDs from images on a real MI355X (`pytest -m gpu`): the fused align-crop kernel against an fp64 restatement of its rule, the
per-channel PReLU against torch, IResNet (reduced depth and the full iresnet100) against an fp32 torch forward of the same modules on the
CPU, and `AdaFaceWrapper.prepare_adaface_embeddings(image_paths)` end to end (INTEGRATION.md "Face IDs from images")."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---- af_face_align_crop ---------------------------------------------------------------------------------------------------------------
def _crop_reference(img, inv_mats, size):
    """The rule of include/adaface_hip.h in fp64: (sx, sy) = inv . (x, y, 1), bilinear over the four neighbours, a tap outside the image
    is 0, (v - 127.5) / 127.5.  Also returns, per output pixel, how many of the four taps lie inside the image."""
    H, W, _ = img.shape
    ys, xs = np.mgrid[0:size, 0:size].astype(np.float64)
    outs, inside = [], []
    for m in np.asarray(inv_mats, dtype=np.float64):
        sx, sy = m[0, 0] * xs + m[0, 1] * ys + m[0, 2], m[1, 0] * xs + m[1, 1] * ys + m[1, 2]
        x0, y0 = np.floor(sx), np.floor(sy)
        ax, ay = (sx - x0)[..., None], (sy - y0)[..., None]
        v, n_in = np.zeros((size, size, 3)), np.zeros((size, size), dtype=np.int64)
        for dy, dx, wgt in ((0, 0, (1 - ay) * (1 - ax)), (0, 1, (1 - ay) * ax), (1, 0, ay * (1 - ax)), (1, 1, ay * ax)):
            xx, yy = (x0 + dx).astype(np.int64), (y0 + dy).astype(np.int64)
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            tap = img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.float64)
            v += wgt * np.where(ok[..., None], tap, 0.0)
            n_in += ok
        outs.append((v - 127.5) / 127.5)
        inside.append(n_in)
    return np.stack(outs), np.stack(inside)


# crop -> image matrices with entries that are not round numbers (fp32 values: the reference reads exactly what the kernel reads)
INV_SMALL = np.array([[[0.2517, -0.0431, 8.313], [0.0431, 0.2517, 3.127]],            # 3.9x magnified, wholly inside the 37 x 53 image
                      [[0.3121, 0.0271, -11.437], [-0.0271, 0.3121, 5.219]],          # the left third of the crop is outside it
                      [[0.3297, 0.0517, 2.711], [-0.0517, 0.3297, 6.193]]],           # 3x magnification
                     dtype=np.float32)
INV_LARGE = np.array([[[2.4937, 0.1763, -5.371], [-0.1763, 2.4937, 21.459]]], dtype=np.float32)          # 2.5x reduction of 301 x 257


@pytest.mark.parametrize("case", ["small", "large", "small128"])
def test_face_align_crop_vs_fp64_rule(dev, case):
    """max |difference| <= 2^-10: the fp16 half-ulp in [0.5, 1] is 2^-11, and the fp32 coordinate error (a few ulp of a coordinate below
    512, ~1e-4 pixel, times a grey-level step of at most 2 in the output's units) stays under the other 2^-11.  The bound is for images
    of at most 512 pixels a side; these are 37 x 53 and 301 x 257."""
    from adaface_dev_amd import ops
    g = np.random.default_rng(41)
    (H, W), inv, size = {"small": ((37, 53), INV_SMALL, 112), "large": ((301, 257), INV_LARGE, 112), "small128": ((37, 53), INV_SMALL[1:2], 128)}[case]
    img = g.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    ref, n_in = _crop_reference(img, inv, size)
    if case == "small":                       # the cases are what they say
        assert n_in[0].min() == 4 and 0.25 < (n_in[1] < 4).mean() < 0.42 and (n_in[1] == 0).any() and (n_in[1] == 4).any()
    out = ops.face_align_crop(torch.from_numpy(img).to(dev), torch.from_numpy(inv).to(dev), size)
    assert out.dtype == torch.float16 and tuple(out.shape) == (len(inv), size, size, 8) and out.is_contiguous()
    got = out.float().cpu().numpy()
    err = float(np.abs(got[..., :3] - ref).max())
    print(f"face_align_crop {case}: max |kernel - fp64 rule| = {err:.3e}")
    assert err <= 2.0 ** -10
    assert (got[..., 3:] == 0).all() and not np.signbit(got[..., 3:]).any()          # exact zeros over NaN-filled memory
    border = n_in == 0
    assert border.any() and (got[..., :3][border] == -1.0).all()                      # all four taps outside: (0 - 127.5) / 127.5


def test_face_align_crop_refuses_bad_arguments(dev):
    from adaface_dev_amd import _lib, ops
    img = torch.zeros((37, 53, 3), dtype=torch.uint8, device=dev)
    inv = torch.from_numpy(INV_SMALL).to(dev)
    assert tuple(ops.face_align_crop(img, inv).shape) == (3, 112, 112, 8)
    bad = [(img.float(), inv, 112), (img.cpu(), inv.cpu(), 112),                      # not uint8; not on the device
           (torch.zeros((37, 106, 3), dtype=torch.uint8, device=dev)[:, ::2], inv, 112),          # not contiguous
           (img.permute(1, 0, 2), inv, 112), (img[..., :2].contiguous(), inv, 112), (img, inv, 96), (img, inv, 64), (img, inv[:0], 112),
           (img, inv.double(), 112), (img, inv[:, :, :2].contiguous(), 112)]
    for a, m, size in bad:
        with pytest.raises(RuntimeError):
            ops.face_align_crop(a, m, size)
    L = _lib.lib()
    out = torch.zeros((1, 128, 128, 8), dtype=torch.float16, device=dev)
    for H, W, nf, size in ((32768, 32768, 1, 112), (26755, 26755, 1, 112), (37, 53, 0, 112), (37, 53, 1, 120)):      # H W 3 >= 2^31; F < 1; size
        assert L.af_face_align_crop(img.data_ptr(), inv.data_ptr(), out.data_ptr(), H, W, nf, size, None) == _lib.AF_E_BADARG
        assert b"af_face_align_crop" in L.af_last_error()
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0                                              # nothing was launched


# ---- af_affine_prelu_ch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", [(5, 8), (35, 72)])
def test_affine_prelu_ch_vs_torch(dev, rows, C):
    from adaface_dev_amd import ops, rng
    x = rng.synth_input("apc.x", (rows, C), seed=71)
    s = 1.0 + 0.2 * rng.synth_input("apc.s", (C,), seed=71)
    t = 0.3 * rng.synth_input("apc.t", (C,), seed=71)
    slope = 0.25 + 0.3 * rng.synth_input("apc.slope", (C,), seed=71)                  # every channel its own, some negative
    xd = x.to(dev).half()
    xh = xd.float().cpu()
    d = lambda v: None if v is None else v.to(dev)
    for sc, sh, sl in ((s, t, slope), (None, None, slope), (s, t, None)):
        y = ops.affine_prelu_ch(xd, d(sc), d(sh), d(sl))
        f = xh if sc is None else xh * sc + sh
        ref = f if sl is None else F.prelu(f, sl)
        assert y.dtype == torch.float16 and y.shape == xd.shape
        assert rel_l2(y.float().cpu().numpy(), ref.numpy()) < 1e-3, (sc is not None, sl is not None)
    y4 = ops.affine_prelu_ch(xd.reshape(1, rows, 1, C), d(s), d(t), d(slope))         # any leading shape: channels are the last axis
    assert torch.equal(y4.reshape(rows, C), ops.affine_prelu_ch(xd, d(s), d(t), d(slope)))
    with pytest.raises(RuntimeError):
        ops.affine_prelu_ch(xd, d(s), d(t), d(slope[:1]))                             # the scalar-slope form is af_affine_prelu's
    with pytest.raises(RuntimeError):
        ops.affine_prelu_ch(xd, d(s), None, d(slope))


# ---- IResNet --------------------------------------------------------------------------------------------------------------------------
def _synth_iresnet(layers, seed, bn3_scale=1.0):
    """Parameters by rng.load_synth_weights, BatchNorm buffers by rng.synth_face_state_dict's rules; bn3_scale multiplies every block's
    bn3.weight.  Returns (module on the CPU, fp32 state dict)."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface.iresnet import IResNet
    with rng.skip_default_init():
        m = IResNet(layers=layers).eval()
    rng.load_synth_weights(m, seed=seed)
    buffers = {k for k, _ in m.named_buffers()}
    synth = rng.synth_face_state_dict({k: v for k, v in m.state_dict().items() if k in buffers}, seed=seed)
    sd = {k: (synth[k] if k in buffers else v.detach().clone()) for k, v in m.state_dict().items()}
    for k in sd:
        if k.endswith(".bn3.weight"):
            sd[k] = sd[k] * bn3_scale
    m.load_state_dict(sd, strict=True)
    return m, sd


def _iresnet_reference(sd, x, layers, block_amax=None):
    """fp32 torch forward of arcface_torch's IResNet in eval mode from the state dict alone."""
    bn = lambda p, h: F.batch_norm(h, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)
    h = F.prelu(bn("bn1", F.conv2d(x, sd["conv1.weight"], None, 1, 1)), sd["prelu.weight"])
    for li, n in enumerate(layers, start=1):
        for bi in range(n):
            p, stride = f"layer{li}.{bi}", (2 if bi == 0 else 1)
            out = bn(p + ".bn2", F.conv2d(bn(p + ".bn1", h), sd[p + ".conv1.weight"], None, 1, 1))
            out = bn(p + ".bn3", F.conv2d(F.prelu(out, sd[p + ".prelu.weight"]), sd[p + ".conv2.weight"], None, stride, 1))
            idt = h if bi else bn(p + ".downsample.1", F.conv2d(h, sd[p + ".downsample.0.weight"], None, stride, 0))
            h = out + idt
            if block_amax is not None:
                block_amax.append(float(h.abs().max()))
    h = F.linear(torch.flatten(bn("bn2", h), 1), sd["fc.weight"], sd["fc.bias"])               # dropout: identity in eval mode
    return F.batch_norm(h, sd["features.running_mean"], sd["features.running_var"], sd["features.weight"], sd["features.bias"], False, 0.0, 1e-5)


def _crops(name, B):
    from adaface_dev_amd import rng
    return rng.synth_input(name, (B, 3, 112, 112), seed=72, scale=0.5).clamp(-1, 1)


def test_iresnet_reduced_depth_vs_fp32_reference(dev):
    """IResNet(layers=(2, 1, 1, 1)), batch 3 and batch 1, with the bounds test_resnet_face18_vs_reference_and_oracle uses for its deeper
    8-block net: rel-L2 < 1e-2, min cosine > 0.9999."""
    layers = (2, 1, 1, 1)
    m, sd = _synth_iresnet(layers, seed=70)
    m = m.to(dev)
    for B in (3, 1):
        x = _crops(f"ir.x{B}", B)
        with torch.no_grad():
            ref = _iresnet_reference(sd, x, layers)
            y = m(x.to(dev))
        assert tuple(y.shape) == (B, 512) and y.dtype == torch.float32
        e, cos = rel_l2(y.cpu().numpy(), ref.numpy()), float(F.cosine_similarity(y.cpu(), ref, dim=-1).min())
        print(f"IResNet{layers} batch {B}: rel-L2 vs fp32 reference {e:.3e}  min cosine {cos:.6f}")
        assert e < 1e-2 and cos > 0.9999
    with torch.no_grad():
        y16 = m(x.to(dev).half())
        assert y16.dtype == torch.float16 and rel_l2(y16.float().cpu().numpy(), ref.numpy()) < 1e-2
        # the aligned-crop entry (NHWC fp16, 8 channels) is the same network
        xn = torch.zeros((1, 112, 112, 8), dtype=torch.float16, device=dev)
        xn[..., :3] = x.to(dev).half().permute(0, 2, 3, 1)
        assert torch.equal(m.forward_nhwc(xn), y16)
        # a weight update invalidates the folded packs
        m.features.bias.add_(1.0)
        assert rel_l2((m(x.to(dev)).cpu() - 1.0).numpy(), ref.numpy()) < 1e-2
    with pytest.raises(NotImplementedError):
        m.train()(x.to(dev))


FULL_DEPTH_REL_L2_MEASURED = 1.574e-3     # MI355X, profiles/face_id_extractor.txt


def test_iresnet100_full_depth_vs_fp32_reference(dev):
    """The full (3, 13, 30, 3) net, batch 2, once.  Weight condition: a random-weight residual net without a final normalisation about
    doubles its variance per block and 49 blocks overflow fp16, so every block's bn3.weight is scaled by 0.2, and the CPU reference must
    show max |activation| < 1e3 at every block output (if it does not, the scale changes, never the bound).  Cosine > 0.999 is the hard
    floor (identity decisions are taken at cosine distances of 0.3 and more); the rel-L2 bound is twice the value measured on the
    MI355X (1.574e-3, min cosine 0.999999), the factor covering box-to-box and batch-order differences of the split-K reductions."""
    layers = (3, 13, 30, 3)
    m, sd = _synth_iresnet(layers, seed=73, bn3_scale=0.2)
    x = _crops("ir.full", 2)
    amax = []
    with torch.no_grad():
        ref = _iresnet_reference(sd, x, layers, amax)
    assert len(amax) == 49 and max(amax) < 1e3, max(amax)
    m = m.to(dev)
    with torch.no_grad():
        y = m(x.to(dev)).cpu()
    e, cos = rel_l2(y.numpy(), ref.numpy()), float(F.cosine_similarity(y, ref, dim=-1).min())
    print(f"iresnet100 batch 2: rel-L2 vs fp32 reference {e:.3e}  min cosine {cos:.6f}  (largest block output {max(amax):.1f})")
    assert bool(torch.isfinite(y).all()) and cos > 0.999
    assert e < 2 * FULL_DEPTH_REL_L2_MEASURED


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
KPS = {1: [[30.3, 41.2], [69.1, 40.4], [50.7, 61.9], [35.2, 80.6], [66.8, 79.3]],
       2: [[52.5, 30.1], [88.4, 36.7], [66.0, 58.3], [49.9, 72.8], [80.2, 78.5]]}


def _photo(tag, seed):
    a = np.random.default_rng(seed).integers(0, 256, size=(96, 120, 3), dtype=np.uint8)
    a[0, 0, 0] = tag
    return a


def _stub_detector(img):
    """Fixed landmarks by the tag in the first pixel; tag 0: nobody in the picture."""
    tag = int(img[0, 0, 0])
    return [] if tag == 0 else [(20.0, 20.0, 60.0, 70.0, 0.9, KPS[tag])]


def test_wrapper_prepares_embeddings_from_images(dev):
    """prepare_adaface_embeddings([img_a, img_b]) is bit-identical to the same call on the IDs the extractor returns for them, with the
    'id_emb' averaging and without; an image set without a face gives None."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper
    from adaface_dev_amd.adaface.arc2face_models import clip_text_config
    from adaface_dev_amd.adaface.face_align import FaceIDExtractor
    net, _ = _synth_iresnet((1, 1, 1, 1), seed=74)
    ex = FaceIDExtractor(net.to(dev), _stub_detector)
    cc = clip_text_config(hidden_size=128, num_attention_heads=2, num_hidden_layers=3, intermediate_size=512)
    w = AdaFaceWrapper(pipeline_name=None, clip_config=cc, device=dev, face_id_extractor=ex)
    assert w.id2ada_prompt_encoder.face_id_extractor is ex
    rng.load_synth_weights(w.text_encoder, seed=60)
    rng.load_synth_weights(w.id2ada_prompt_encoder.text_to_image_prompt_encoder, seed=61)
    rng.load_synth_weights(w.id2ada_prompt_encoder.subj_basis_generator.prompt2token_proj, seed=62)
    w = w.to(dev)
    img_a, img_b, nobody = _photo(1, 5), _photo(2, 6), _photo(0, 7)
    faceless, ids = ex.extract([img_a, img_b])
    assert faceless == 0 and tuple(ids.shape) == (2, 512) and ids.dtype == torch.float32 and ids.device.type == "cuda"
    assert torch.allclose(ids.norm(dim=-1), torch.ones(2, device=dev), atol=1e-5)
    assert float(F.cosine_similarity(ids[0], ids[1], dim=0)) < 0.9999                 # two crops, two IDs
    for avg, images, kw in (("id_emb", [img_a, img_b], {}), (None, [img_a], {}),
                            (None, [img_a, img_b], dict(update_text_encoder=False))):       # (the token table takes one subject's 16 rows)
        given = ex.extract(images, calc_avg=(avg == "id_emb"))[1]
        assert tuple(given.shape) == ((1, 512) if avg else (len(images), 512))
        from_images = w.prepare_adaface_embeddings(images, avg_at_stage=avg, **kw)
        from_ids = w.prepare_adaface_embeddings(None, face_id_embs=given, avg_at_stage=avg, **kw)
        assert from_images is not None and bool(torch.isfinite(from_images.float()).all())
        assert from_images.shape == from_ids.shape and torch.equal(from_images, from_ids), (avg, len(images))
    assert tuple(from_images.shape) == (2, 16, 128)
    table = w.text_encoder.text_model.embeddings.token_embedding.weight.detach().clone()
    assert w.prepare_adaface_embeddings([nobody, nobody]) is None
    assert torch.equal(table, w.text_encoder.text_model.embeddings.token_embedding.weight)          # nothing was written
