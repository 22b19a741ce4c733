"""The RetinaFace detector on a real MI355X (`pytest -m gpu`): the small kernels of af_detect.hip against torch on the CPU from the same
values, decode + NMS against the fp64 restatement of include/adaface_hip.h (tests/retina_reference.py), the network's head tensors against an
fp32 torch forward built from the state dict alone, and the detector end to end through `FaceIDExtractor` and `FaceCropper`
(INTEGRATION.md "Face detector")."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import retina_reference as R
from adaface_dev_amd.adaface.retinaface import PREPROCESS, RetinaFaceDetector
from conftest import rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _affine(preset):
    d = RetinaFaceDetector(None, preprocess=preset)
    return d.scale, d.shift, d.bgr


# ---- the small kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 37, 53), (2, 64, 96)])
@pytest.mark.parametrize("preset", ["biubug6", "ternaus"])
def test_stem_im2col_vs_fp64_unfold(dev, shape, preset):
    """max |difference| <= the fp16 half-ulp of the largest normalised magnitude.  The kernel forms v * scale + shift in fp32 (relative
    error 2^-23, nothing beside fp16's 2^-11) and rounds once, so against the fp64 value the error is at most half an fp16 ulp of the
    result: with biubug6's preset |v - mean| <= 255 - 104 = 151 lies in [128, 256), ulp 2^-3, half-ulp 2^-4; with ternaus' preset
    |(v - mean) / std| <= (255 - 0.406 * 255) / (0.225 * 255) = 2.64 lies in [2, 4), ulp 2^-9, half-ulp 2^-10.  The bound is computed from
    the reference's own largest magnitude (plus the fp32 term)."""
    from adaface_dev_amd import ops
    B, H, W = shape
    img = np.random.default_rng(43).integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    img[0, 0, 0], img[0, -1, -1] = 255, 0                                    # the extremes of every channel are present
    scale, shift, bgr = _affine(preset)
    mean, std, _ = PREPROCESS[preset]
    x = R.normalise_and_pad(img, mean, std, bgr, dtype=torch.float64)
    Hp, Wp = x.shape[2:]
    ref = F.unfold(x, 7, padding=3, stride=2)                                # [B, 3 * 49, Ho * Wo], rows (c, ky, kx)
    ref = ref.reshape(B, 3, 49, -1).permute(0, 3, 2, 1).reshape(-1, 147).numpy()          # -> rows of pixels, columns (ky, kx, c)
    rows, (Ho, Wo) = ops.stem_im2col7x7(torch.from_numpy(img).to(dev), scale, shift, bgr)
    assert (Ho, Wo) == (Hp // 2, Wp // 2) and tuple(rows.shape) == (B * Ho * Wo, 160) and rows.dtype == torch.float16
    got = rows.float().cpu().numpy()
    amax = float(np.abs(ref).max())
    half_ulp = 2.0 ** (np.floor(np.log2(amax)) - 11)
    err = float(np.abs(got[:, :147] - ref).max())
    print(f"stem_im2col7x7 {shape} {preset}: max |kernel - fp64| = {err:.3e}, fp16 half-ulp at {amax:.2f} = {half_ulp:.3e}")
    assert err <= half_ulp * (1 + 2.0 ** -10)
    assert (got[:, 147:] == 0).all() and not np.signbit(got[:, 147:]).any()


def test_stem_im2col_pad_columns_over_nan_memory(dev):
    """Columns 147-159 are exact zeros when the output lands on NaN-filled memory (the GEMM multiplies them by zero weights)."""
    from adaface_dev_amd import _lib
    img = torch.zeros((1, 37, 53, 3), dtype=torch.uint8, device=dev)
    out = torch.full((32 * 32 * 160,), float("nan"), dtype=torch.float16, device=dev)
    import ctypes
    f3 = ctypes.c_float * 3
    assert _lib.lib().af_stem_im2col7x7(img.data_ptr(), f3(1, 1, 1), f3(-104, -117, -123), out.data_ptr(), 1, 37, 53, 1, None) == 0
    got = out.reshape(32 * 32, 160).float().cpu()
    assert bool(torch.isfinite(got).all()) and bool((got[:, 147:] == 0).all())
    assert float(got[0, 0]) == 0.0 and float(got[0, 3 * 21 + 3 * 3]) == -104.0           # tap (-3, -3) is outside; the centre tap is pixel (0, 0)


@pytest.mark.parametrize("shape", [(2, 9, 13, 64), (1, 16, 16, 8)])
def test_relu_maxpool_bit_exact(dev, shape):
    from adaface_dev_amd import ops, rng
    x = rng.synth_input("rf.pool", shape, seed=81).half()
    x[0, :2, :2, :] = -x[0, :2, :2, :].abs() - 0.5                           # an all-negative window at a corner: the padding must not win
    ref = F.relu(F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1)).permute(0, 2, 3, 1)
    assert float(ref[0, 0, 0].max()) == 0.0
    y = ops.relu_maxpool3x3s2(x.to(dev))
    assert y.dtype == torch.float16 and y.is_contiguous() and torch.equal(y.float().cpu(), ref)


@pytest.mark.parametrize("shape", [(2, 7, 9, 16), (1, 8, 6, 264)])
def test_subsample_bit_exact(dev, shape):
    from adaface_dev_amd import ops, rng
    x = rng.synth_input("rf.sub", shape, seed=82).half()
    y = ops.subsample2x(x.to(dev))
    assert torch.equal(y.cpu(), x[:, ::2, ::2, :].contiguous())


def test_upsample_add_bit_exact(dev):
    from adaface_dev_amd import ops, rng
    a, b = rng.synth_input("rf.up.a", (2, 4, 6, 256), seed=83).half(), rng.synth_input("rf.up.b", (2, 2, 3, 256), seed=83).half()
    ref = (a.float() + b.float().repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)).half()
    assert torch.equal(ops.upsample2x_add(a.to(dev), b.to(dev)).cpu(), ref)
    with pytest.raises(RuntimeError):
        ops.upsample2x_add(a.to(dev), a.to(dev))


# ---- decode + NMS ---------------------------------------------------------------------------------------------------------------------
CONF_THR, NMS_THR = 0.6, 0.4


def planted_heads(H, W, seed, n_pass=100):
    """fp16 head tensors [2, HkWk, 32] for an H x W image.  Box / landmark logits uniform in [-4, 4] (|0.2 box| <= 0.8 <= 1).  Image 0:
    ``n_pass`` anchors get cls1 - cls0 in [0.7, 4] (scores 0.67 .. 0.98), the rest in [-4, -0.7] (scores <= 0.33), and two passing anchors
    are given the same class logits (the anchor-index tie-break); image 1: none passes."""
    g = np.random.default_rng(seed)
    sizes = R.level_sizes(H, W)
    A = 2 * sum(hk * wk for hk, wk in sizes)
    v = g.uniform(-4, 4, size=(2, A, 16))
    v[..., 4] = 0.0
    v[..., 5] = -g.uniform(0.7, 4, size=(2, A))
    chosen = g.choice(A, size=n_pass, replace=False)
    v[0, chosen, 5] = g.uniform(0.7, 4, size=n_pass)
    v[0, chosen[1], 5] = v[0, chosen[0], 5]
    v = torch.from_numpy(v).half()
    heads, o = [], 0
    for hk, wk in sizes:
        heads.append(v[:, o:o + 2 * hk * wk].reshape(2, hk * wk, 32).contiguous())
        o += 2 * hk * wk
    return heads, sizes


def _reference(heads, sizes, b, conf_thr, nms_thr, max_det):
    return R.nms_reference(R.decode_pixels([h[b].double().numpy() for h in heads], sizes), conf_thr, nms_thr, max_det)


def check_input_conditions(heads, sizes, max_det, want_chain):
    """The conditions the comparison rests on, asserted on the reference itself (tests/test_retinaface_host.py checks the seeds without a
    GPU): no score within 1e-3 of the threshold, no pairwise IoU among passing anchors within 1e-3 of the NMS threshold, two equal scores,
    and a suppression chain (a suppressed box that would itself have suppressed a kept one)."""
    rows = R.decode_pixels([h[0].double().numpy() for h in heads], sizes)
    assert np.abs(rows[:, 4] - CONF_THR).min() > 1e-3
    kept, passing, p, iou = R.nms_reference(rows, CONF_THR, NMS_THR, max_det)
    assert 90 <= passing <= 110 and np.abs(iou - NMS_THR).min() > 1e-3
    assert len(np.unique(p[:, 4])) < passing                                  # equal scores: the anchor index decides
    full, _, _, _ = R.nms_reference(rows, CONF_THR, NMS_THR, 1024)
    kept_idx = set(full[:, 15].astype(int))
    order = {int(a): i for i, a in enumerate(p[:, 15])}
    dead = [i for i in range(passing) if int(p[i, 15]) not in kept_idx]
    chain = any(iou[j, order[k]] > NMS_THR for j in dead for k in kept_idx if order[k] > j)
    assert chain or not want_chain
    assert R.nms_reference(R.decode_pixels([h[1].double().numpy() for h in heads], sizes), CONF_THR, NMS_THR, max_det)[1] == 0
    return len(full)


CASES = {"64x96": (64, 96, 96, 64), "96x64_maxdet8": (96, 64, 96, 8)}


@pytest.mark.parametrize("case", list(CASES))
def test_decode_nms_vs_fp64_restatement(dev, case):
    """Coordinates: |difference| <= 1e-2 pixel (they stay below ~1.5e3, an fp32 ulp there is ~1e-4; a handful of operations and a fast exp
    stay two orders of magnitude under the bound, while a wrong variance, step or order is off by pixels).  Scores: <= 1e-5.  The kept anchor
    indices and the counts are EQUAL to the reference's, the result is bit-identical over two runs and rows beyond `kept` are zero."""
    from adaface_dev_amd import ops
    H, W, seed, max_det = CASES[case]
    heads, sizes = planted_heads(H, W, seed)
    n_full = check_input_conditions(heads, sizes, max_det, want_chain=True)
    assert n_full > 8 and (max_det == 64 or n_full > max_det)
    hd = [h.to(dev) for h in heads]
    runs = []
    for _ in range(2):
        cand, count = ops.retina_decode(hd, sizes, CONF_THR)
        runs.append(ops.retina_nms(cand, count, NMS_THR, max_det))
    (table, counts), (table2, counts2) = runs
    assert torch.equal(table, table2) and torch.equal(counts, counts2)
    assert tuple(table.shape) == (2, max_det, 16) and table.dtype == torch.float32 and counts.dtype == torch.int32
    for b in range(2):
        kept, passing, _, _ = _reference(heads, sizes, b, CONF_THR, NMS_THR, max_det)
        assert counts[b].tolist() == [len(kept), passing]
        got = table[b].double().numpy()
        assert (got[len(kept):] == 0).all()
        if not len(kept):
            continue
        assert (got[:len(kept), 15] == kept[:, 15]).all()
        e_xy = float(np.abs(np.delete(got[:len(kept), :15], 4, axis=1) - np.delete(kept[:, :15], 4, axis=1)).max())
        e_s = float(np.abs(got[:len(kept), 4] - kept[:, 4]).max())
        print(f"decode + nms {case} image {b}: kept {len(kept)} of {passing} passing; max coordinate error {e_xy:.3e} px, score error {e_s:.3e}")
        assert e_xy <= 1e-2 and e_s <= 1e-5
    if max_det == 8:
        assert counts[0, 0] == 8


def test_decode_reports_overflow_and_wrapper_raises(dev):
    """1100 passing anchors at synthetic level sizes 24 x 32, 12 x 16, 6 x 8 (2016 anchors): the count says 1100, the list holds 1024, and
    the wrapper raises instead of returning a list whose content depends on scheduling."""
    from adaface_dev_amd import _lib, ops
    g = np.random.default_rng(93)
    sizes = [(24, 32), (12, 16), (6, 8)]
    A = 2 * sum(h * w for h, w in sizes)
    v = g.uniform(-1, 1, size=(1, A, 16))
    v[..., 4], v[..., 5] = 0.0, -3.0
    v[0, g.choice(A, size=1100, replace=False), 5] = 3.0
    v = torch.from_numpy(v).half()
    heads, o = [], 0
    for h, w in sizes:
        heads.append(v[:, o:o + 2 * h * w].reshape(1, h * w, 32).contiguous().to(dev))
        o += 2 * h * w
    cand, count = ops.retina_decode(heads, sizes, CONF_THR)
    assert count.tolist() == [1100]
    with pytest.raises(RuntimeError, match="raise the confidence threshold"):
        ops.retina_nms(cand, count, NMS_THR, 64)
    out, oc = torch.zeros((64, 16), device=dev), torch.zeros((2,), dtype=torch.int32, device=dev)
    assert _lib.lib().af_retina_nms(cand.data_ptr(), count.data_ptr(), out.data_ptr(), oc.data_ptr(), 1, 1024, 64, NMS_THR, None) == 0
    assert int(oc[1]) == 1100 and 1 <= int(oc[0]) <= 64
    anchors = cand[0, :, 15].cpu().numpy()
    assert len(np.unique(anchors)) == 1024 and (v[0, anchors.astype(int), 5] == 3.0).all()          # 1024 distinct passing anchors made the list


# ---- the network ------------------------------------------------------------------------------------------------------------------------
def _images(B, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)


def _heads_vs_reference(m, sd, layers, img, preset, dev, amax=None):
    scale, shift, bgr = _affine(preset)
    mean, std, _ = PREPROCESS[preset]
    with torch.no_grad():
        ref = R.retina_reference(sd, R.normalise_and_pad(img, mean, std, bgr), layers, amax)
        heads, sizes = m.forward_heads(torch.from_numpy(img).to(dev), scale, shift, bgr)
    Hp, Wp = -(-img.shape[1] // 32) * 32, -(-img.shape[2] // 32) * 32
    assert sizes == [(Hp // s, Wp // s) for s in (8, 16, 32)]
    out = []
    for k, (h, r) in enumerate(zip(heads, ref)):
        assert h.dtype == torch.float16 and tuple(h.shape) == tuple(r.shape)
        hc = h.float().cpu()
        out.append((rel_l2(hc.numpy(), r.numpy()), float(F.cosine_similarity(hc.flatten(), r.flatten(), dim=0))))
    return out


def test_retinaface_reduced_depth_vs_fp32_reference(dev):
    """RetinaFace(layers=(1, 1, 1, 1)) with both presets at (2, 64, 96) and (1, 37, 53), with the project's bound for the face networks:
    rel-L2 < 1e-2 on each level's [., 32] head tensor."""
    layers = (1, 1, 1, 1)
    m, sd = R.synth_retinaface(layers, seed=84)
    m = m.to(dev)
    for (B, H, W), preset in (((2, 64, 96), "biubug6"), ((1, 37, 53), "ternaus"), ((1, 37, 53), "biubug6")):
        img = _images(B, H, W, seed=85)
        for k, (e, cos) in enumerate(_heads_vs_reference(m, sd, layers, img, preset, dev)):
            print(f"RetinaFace{layers} {preset} {(B, H, W)} level {k}: rel-L2 vs fp32 reference {e:.3e}  cosine {cos:.6f}")
            assert e < 1e-2
    # a weight update invalidates the folded packs
    img = _images(1, 37, 53, seed=85)
    scale, shift, bgr = _affine("ternaus")
    with torch.no_grad():
        before, _ = m.forward_heads(torch.from_numpy(img).to(dev), scale, shift, bgr)
        m.BboxHead[0].conv1x1.bias.add_(1.0)
        after, _ = m.forward_heads(torch.from_numpy(img).to(dev), scale, shift, bgr)
    d = (after[0].float() - before[0].float()).reshape(-1, 2, 16)
    ulp = 2.0 ** (np.floor(np.log2(float(after[0].float().abs().max()))) - 10)          # fp16 spacing at the largest head value
    assert float((d[..., :4] - 1.0).abs().max()) <= ulp and float(d[..., 4:].abs().max()) == 0.0 and torch.equal(after[1], before[1])
    with pytest.raises(NotImplementedError):
        m.train().forward_heads(torch.from_numpy(img).to(dev), scale, shift, bgr)


FULL_DEPTH_BN3_SCALE = 1.0
FULL_DEPTH_REL_L2_MEASURED = 9.180e-4     # the largest of the three levels, MI355X, profiles/retinaface_detector.txt


def test_retinaface_r50_full_depth_vs_fp32_reference(dev):
    """The full (3, 4, 6, 3) network, batch 2 at 64 x 64, once.  Weight condition: a random-weight residual network about doubles its
    variance per block, so every Bottleneck's bn3.weight is scaled by FULL_DEPTH_BN3_SCALE and the CPU reference must show
    max |activation| < 1e3 at every block output (if it does not, the scale changes, never the bound).  Cosine > 0.999 per level is the hard
    floor; the rel-L2 bound is twice the largest per-level value measured on the MI355X (9.180e-4, 7.909e-4, 8.743e-4 for strides 8, 16, 32,
    cosine 0.999999 and better; with scale 1.0 the reference's largest block output is 11.9, so the weights stay as drawn)."""
    layers = (3, 4, 6, 3)
    m, sd = R.synth_retinaface(layers, seed=86, bn3_scale=FULL_DEPTH_BN3_SCALE)
    img = _images(2, 64, 64, seed=87)
    amax = []
    res = _heads_vs_reference(m.to(dev), sd, layers, img, "ternaus", dev, amax)
    assert len(amax) == 16 and max(amax) < 1e3, max(amax)
    for k, (e, cos) in enumerate(res):
        print(f"RetinaFace-R50 batch 2 level {k}: rel-L2 vs fp32 reference {e:.3e}  cosine {cos:.6f}  (largest block output {max(amax):.1f})")
    for e, cos in res:
        assert cos > 0.999
        assert e < 2 * FULL_DEPTH_REL_L2_MEASURED


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def _threshold_for(rows_per_image, lo, hi):
    """A confidence threshold in the widest score gap that lets between lo and hi anchors of every image's reference pass."""
    s = np.sort(np.concatenate([r[:, 4] for r in rows_per_image]))[::-1]
    best = max(range(lo, hi), key=lambda k: s[k - 1] - s[k])
    return float((s[best - 1] + s[best]) / 2)


@pytest.fixture(scope="module")
def small_net(dev):
    m, _ = R.synth_retinaface((1, 1, 1, 1), seed=88)
    return m.to(dev)


def _own_rows(det, img):
    """The fp64 decode of the detector's own head tensors for img [B, H, W, 3]."""
    with torch.no_grad():
        heads, sizes = det.model.forward_heads(torch.from_numpy(img).to(det.device), det.scale, det.shift, det.bgr)
    return [R.decode_pixels([h[b].double().cpu().numpy() for h in heads], sizes) for b in range(img.shape[0])]


def test_detector_end_to_end_vs_reference_on_its_own_heads(dev, small_net):
    """det(image) on a 96 x 120 image = the fp64 decode + NMS of the detector's own head tensors (pinned above), in image pixels: pins
    level order, padding offsets and the adapter.  The confidence threshold is put into a score gap of the reference so that between 3 and 50
    anchors pass."""
    img = _images(1, 96, 120, seed=89)[0]
    det = RetinaFaceDetector(small_net, preprocess="ternaus")
    rows = _own_rows(det, img[None])
    det.conf_threshold = _threshold_for(rows, 3, 50)
    kept, passing, _, _ = R.nms_reference(rows[0], det.conf_threshold, det.nms_threshold, det.max_det)
    assert 3 <= passing <= 50 and len(kept) >= 1
    faces = det(img)
    print(f"end to end: threshold {det.conf_threshold:.4f}, {passing} passing, {len(kept)} kept")
    assert len(faces) == len(kept)
    for f, r in zip(faces, kept):
        assert len(f) == 6
        got = np.array([f[0], f[1], f[0] + f[2], f[1] + f[3]] + [c for pt in f[5] for c in pt])
        assert np.abs(got - np.delete(r[:15], 4)).max() <= 1e-2 and abs(f[4] - r[4]) <= 1e-5
    boxes = det.detect_boxes(img)
    assert [b[:4] for b in boxes] == [f[:4] for f in faces] and all(len(b) == 5 for b in boxes)


def test_detector_feeds_face_id_extractor_and_face_cropper(dev, small_net):
    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface.face_align import FaceIDExtractor
    from adaface_dev_amd.adaface.iresnet import IResNet
    from adaface_dev_amd.ldm.modules.arcface_wrapper import FaceCropper, images_to_uint8
    det = RetinaFaceDetector(small_net, preprocess="ternaus")
    img = _images(1, 96, 120, seed=89)[0]
    det.conf_threshold = _threshold_for(_own_rows(det, img[None]), 3, 50)
    with rng.skip_default_init():
        net = IResNet(layers=(1, 1, 1, 1)).eval()
    rng.load_synth_weights(net, seed=74)
    faceless, ids = FaceIDExtractor(net.to(dev), det).extract([img])
    assert faceless == 0 and tuple(ids.shape) == (1, 512) and abs(float(ids.norm()) - 1.0) < 1e-5
    # FaceCropper: its own rule applied to det.detect_boxes' output gives the boxes it returns
    images = rng.synth_input("rf.crop", (2, 3, 64, 96), seed=90, scale=0.5).clamp(-1, 1)
    u8 = images_to_uint8(images)
    det.conf_threshold = _threshold_for(_own_rows(det, u8), 40, 200)
    T, (H, W) = 20, images.shape[2:]
    fg, bg, boxes, conf, found = FaceCropper(detect_faces=det.detect_boxes).crop_faces(images.to(dev), out_size=(32, 32), T=T)
    assert int(found.sum()) >= 1 and tuple(fg.shape) == (2, 3, 32, 32)
    for b in range(2):
        cands = []
        for (x, y, w, h, c) in det.detect_boxes(u8[b], T):
            x0, y0, x1, y1 = max(0, int(x)), max(0, int(y)), min(W, int(x + w)), min(H, int(y + h))
            if h > T and w > T and y0 + T < y1 and x0 + T < x1:
                cands.append(((y1 - y0) * (x1 - x0), c, x0, y0, x1, y1))
        assert bool(found[b]) == bool(cands)
        if cands:
            best = max(cands, key=lambda r: r[0])
            assert boxes[b].tolist() == list(best[2:]) and abs(float(conf[b]) - best[1]) < 1e-6
