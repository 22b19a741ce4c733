"""The RetinaFace detector, the host side (no GPU): the module tree and checkpoint naming of `adaface/retinaface.py`, the anchor order and
the pixel-space decode rules against a numpy port of biubug6's PriorBox / decode / decode_landm, `RetinaFaceDetector`'s two adapters with a
stubbed `detect_batch`, and the C ABI's argument checks (INTEGRATION.md "Face detector").  The kernels and the network's arithmetic are
pinned on the GPU in tests/test_hip_retinaface.py."""
import numpy as np
import pytest
import torch

import retina_reference as R
from adaface_dev_amd.adaface.retinaface import RetinaFace, RetinaFaceDetector, load_retinaface_state_dict

SPOT_KEYS = {
    "body.conv1.weight": (64, 3, 7, 7), "body.bn1.running_mean": (64,),
    "body.layer1.0.conv1.weight": (64, 64, 1, 1), "body.layer1.0.conv2.weight": (64, 64, 3, 3), "body.layer1.0.conv3.weight": (256, 64, 1, 1),
    "body.layer1.0.downsample.0.weight": (256, 64, 1, 1), "body.layer1.2.bn3.weight": (256,),
    "body.layer2.0.downsample.0.weight": (512, 256, 1, 1), "body.layer2.3.conv2.weight": (128, 128, 3, 3),
    "body.layer3.5.conv3.weight": (1024, 256, 1, 1), "body.layer3.0.downsample.1.running_var": (1024,),
    "body.layer4.2.conv3.weight": (2048, 512, 1, 1), "body.layer4.0.conv1.weight": (512, 1024, 1, 1),
    "fpn.output1.0.weight": (256, 512, 1, 1), "fpn.output3.0.weight": (256, 2048, 1, 1), "fpn.merge2.0.weight": (256, 256, 3, 3),
    "fpn.merge1.1.bias": (256,),
    "ssh1.conv3X3.0.weight": (128, 256, 3, 3), "ssh2.conv5X5_1.0.weight": (64, 256, 3, 3), "ssh2.conv5X5_2.1.weight": (64,),
    "ssh3.conv7X7_2.0.weight": (64, 64, 3, 3), "ssh3.conv7x7_3.1.running_var": (64,),
    "ClassHead.0.conv1x1.weight": (4, 256, 1, 1), "BboxHead.1.conv1x1.weight": (8, 256, 1, 1), "LandmarkHead.2.conv1x1.bias": (20,),
}


def _expected_keys():
    """The key set of biubug6's RetinaFace(cfg_re50), written out from the architecture."""
    bnk = lambda p: [f"{p}.{s}" for s in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    keys = ["body.conv1.weight"] + bnk("body.bn1")
    for li, n in zip((1, 2, 3, 4), (3, 4, 6, 3)):
        for bi in range(n):
            p = f"body.layer{li}.{bi}"
            for c in (1, 2, 3):
                keys += [f"{p}.conv{c}.weight"] + bnk(f"{p}.bn{c}")
            if bi == 0:
                keys += [f"{p}.downsample.0.weight"] + bnk(f"{p}.downsample.1")
    for n in ("output1", "output2", "output3", "merge1", "merge2"):
        keys += [f"fpn.{n}.0.weight"] + bnk(f"fpn.{n}.1")
    for k in (1, 2, 3):
        for n in ("conv3X3", "conv5X5_1", "conv5X5_2", "conv7X7_2", "conv7x7_3"):
            keys += [f"ssh{k}.{n}.0.weight"] + bnk(f"ssh{k}.{n}.1")
    for h in ("ClassHead", "BboxHead", "LandmarkHead"):
        for k in range(3):
            keys += [f"{h}.{k}.conv1x1.weight", f"{h}.{k}.conv1x1.bias"]
    return keys


def test_module_tree_is_biubug6_cfg_re50():
    m = RetinaFace()
    sd = m.state_dict()
    assert sorted(sd) == sorted(_expected_keys())
    for k, shape in SPOT_KEYS.items():
        assert tuple(sd[k].shape) == shape, k
    # ResNet-50 without fc (23,508,032) + FPN + 3 SSH + 9 head convolutions
    assert sum(p.numel() for p in m.parameters()) == 27_293_600
    assert m.inference_only and not m.training and not any(p.requires_grad for p in m.parameters())
    # a DataParallel checkpoint (Resnet50_Final.pth) loads strictly through the helper, a plain one (ternaus) too; a missing key raises
    ck = {"module." + k: torch.full_like(v, 0.5) if v.is_floating_point() else v.clone() for k, v in sd.items()}
    load_retinaface_state_dict(m, ck)
    assert float(m.state_dict()["ssh3.conv7x7_3.1.running_var"][0]) == 0.5
    load_retinaface_state_dict(m, {k[len("module."):]: v for k, v in ck.items()})
    ck.pop("module.fpn.merge2.0.weight")
    with pytest.raises(RuntimeError):
        load_retinaface_state_dict(m, ck)
    with pytest.raises(RuntimeError, match="CPU"):
        m.forward_heads(torch.zeros((1, 32, 32, 3), dtype=torch.uint8), (1, 1, 1), (0, 0, 0))
    r = RetinaFace(layers=(1, 1, 1, 1), out_channel=64)
    assert r.fpn.output1[2].negative_slope == 0.1 and m.fpn.output1[2].negative_slope == 0.0
    assert tuple(r.state_dict()["ssh1.conv7x7_3.0.weight"].shape) == (16, 16, 3, 3)


@pytest.mark.parametrize("H,W", [(64, 96), (96, 64)])
def test_pixel_decode_is_biubug6_priorbox_and_decode(H, W):
    """biubug6's PriorBox + decode + decode_landm in normalised units, scaled by (W, H), against the pixel-space formulas of
    include/adaface_hip.h, both in fp64: pins the anchor order (level, row, column, min-size) and the restatement."""
    g = np.random.default_rng(5)
    sizes = R.level_sizes(H, W)
    heads = [g.standard_normal((hk * wk, 32)) for hk, wk in sizes]
    per_anchor = np.concatenate([h.reshape(-1, 16) for h in heads])
    priors = R.priorbox_biubug6(H, W)
    assert len(priors) == len(per_anchor) == 2 * sum(hk * wk for hk, wk in sizes) == 252
    boxes = R.decode_biubug6(per_anchor[:, :4], priors) * np.array([W, H, W, H])
    ldm = R.decode_landm_biubug6(per_anchor[:, 6:], priors) * np.array([W, H] * 5)
    e = np.exp(per_anchor[:, 4:6] - per_anchor[:, 4:6].max(axis=1, keepdims=True))
    score = e[:, 1] / e.sum(axis=1)                                          # F.softmax(conf, dim=-1)[:, 1]
    rows = R.decode_pixels(heads, sizes)
    assert np.abs(rows[:, :4] - boxes).max() < 1e-9 and np.abs(rows[:, 5:15] - ldm).max() < 1e-9
    assert np.abs(rows[:, 4] - score).max() < 1e-9 and (rows[:, 15] == np.arange(252)).all()


class _StubModel:
    class body:
        class conv1:
            weight = torch.zeros(1)


def _stub_detector(table_rows, monkeypatch, **kw):
    det = RetinaFaceDetector(_StubModel(), **kw)
    seen = []

    def detect_batch(images_u8):
        seen.append(tuple(images_u8.shape))
        t = torch.zeros((1, det.max_det, 16))
        t[0, :len(table_rows)] = torch.tensor(table_rows, dtype=torch.float32)
        return t, torch.tensor([[len(table_rows), len(table_rows) + 3]], dtype=torch.int32)

    monkeypatch.setattr(det, "detect_batch", detect_batch)
    return det, seen


ROWS = [[10.0, 12.0, 50.0, 72.0, 0.95] + [20.0, 30.0, 40.0, 30.5, 30.0, 45.0, 22.0, 60.0, 38.0, 60.5] + [7.0],
        [60.0, 5.0, 80.0, 31.0, 0.80] + [65.0, 12.0, 75.0, 12.5, 70.0, 18.0, 66.0, 25.0, 74.0, 25.5] + [3.0]]


def test_adapters_contracts_and_scaling(monkeypatch):
    det, seen = _stub_detector(ROWS, monkeypatch)
    img = np.zeros((96, 120, 3), dtype=np.uint8)
    faces = det(img)
    assert seen == [(1, 96, 120, 3)] and len(faces) == 2 and all(len(f) == 6 for f in faces)
    x, y, w, h, c, kps = faces[0]
    assert (x, y, w, h) == (10.0, 12.0, 40.0, 60.0) and abs(c - 0.95) < 1e-6 and np.asarray(kps).shape == (5, 2)
    assert kps[0] == [20.0, 30.0] and kps[4] == [38.0, 60.5]
    boxes = det.detect_boxes(img, 20)
    assert [len(b) for b in boxes] == [5, 5] and boxes[1][:4] == (60.0, 5.0, 20.0, 26.0)
    # a 2048 x 1024 image (W x H) with max_size = 1024 is halved on the host and its detections doubled; a smaller one is never enlarged
    det, seen = _stub_detector(ROWS, monkeypatch, max_size=1024)
    faces = det(np.zeros((1024, 2048, 3), dtype=np.uint8))
    assert seen == [(1, 512, 1024, 3)]
    assert faces[0][:4] == (20.0, 24.0, 80.0, 120.0) and abs(faces[0][4] - 0.95) < 1e-6 and faces[0][5][4] == [76.0, 121.0]
    det(np.zeros((40, 30, 3), dtype=np.uint8))
    assert seen[-1] == (1, 40, 30, 3)
    with pytest.raises(ValueError):
        RetinaFaceDetector(_StubModel(), preprocess="imagenet")
    # the presets: network channel order and the affine the stem kernel applies
    b, t = RetinaFaceDetector(_StubModel()), RetinaFaceDetector(_StubModel(), preprocess="ternaus")
    assert b.bgr and b.scale == (1.0, 1.0, 1.0) and b.shift == (-104.0, -117.0, -123.0)
    assert not t.bgr and np.allclose(t.scale, [1 / (255 * s) for s in (0.229, 0.224, 0.225)])
    assert np.allclose(t.shift, [-m / s for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))])
    c = RetinaFaceDetector(_StubModel(), preprocess=((10.0, 20.0, 30.0), (2.0, 4.0, 5.0), True))
    assert c.scale == (0.2, 0.25, 0.5) and c.shift == (-6.0, -5.0, -5.0)


def test_adapters_drive_face_cropper_and_face_id_extractor(monkeypatch):
    from adaface_dev_amd.adaface.face_align import FaceIDExtractor
    from adaface_dev_amd.ldm.modules.arcface_wrapper import FaceCropper
    det, seen = _stub_detector(ROWS, monkeypatch)
    images = torch.zeros((2, 3, 96, 120))
    fg, bg, boxes, conf, found = FaceCropper(detect_faces=det.detect_boxes).crop_faces(images, out_size=(32, 32), T=20)
    assert tuple(fg.shape) == (2, 3, 32, 32) and found.tolist() == [1, 1] and boxes.tolist() == [[10, 12, 50, 72]] * 2
    assert torch.allclose(conf, torch.tensor([0.95, 0.95])) and bg is None          # the 20 x 26 face falls to w <= T
    assert len(seen) == 2
    # FaceIDExtractor: the largest face's landmarks reach the crop
    from adaface_dev_amd import ops
    crops = []
    monkeypatch.setattr(ops, "face_align_crop", lambda img, inv, size: crops.append(inv.clone()) or torch.zeros((1, size, size, 8)))
    ex = FaceIDExtractor(lambda c: torch.ones((c.shape[0], 512)), det, device="cpu")
    faceless, ids = ex.extract([np.zeros((96, 120, 3), dtype=np.uint8)])
    assert faceless == 0 and tuple(ids.shape) == (1, 512) and len(crops) == 1
    from adaface_dev_amd.adaface.face_align import estimate_similarity
    assert np.allclose(crops[0][0].numpy(), estimate_similarity(np.array(ROWS[0][5:15]).reshape(5, 2))[1], atol=1e-5)


def test_c_abi_refuses_bad_detector_arguments_before_any_launch():
    """Argument validation precedes the launch, so it is observable without a GPU (the device pointers are never dereferenced)."""
    import ctypes
    from adaface_dev_amd import _lib
    L = _lib.lib()
    E = _lib.AF_E_BADARG
    f3, i3, i6, f6 = ctypes.c_float * 3, ctypes.c_int * 3, ctypes.c_int * 6, ctypes.c_float * 6
    sc, sh = f3(1, 1, 1), f3(0, 0, 0)
    named = lambda name: name.encode() in L.af_last_error()
    for args in ((None, sc, sh, 4096, 1, 64, 96, 0), (4096, None, sh, 4096, 1, 64, 96, 0), (4096, sc, sh, None, 1, 64, 96, 0),
                 (4096, sc, sh, 4100, 1, 64, 96, 0), (4096, sc, sh, 4096, 0, 64, 96, 0), (4096, sc, sh, 4096, 1, 0, 96, 0),
                 (4096, sc, sh, 4096, 1, 32768, 32768, 0), (4096, sc, sh, 4096, 64, 2048, 2048, 0)):      # B H W 3 >= 2^31; B Ho Wo 320 >= 2^31
        assert L.af_stem_im2col7x7(*args, None) == E and named("af_stem_im2col7x7"), args
    for fn, name in ((L.af_relu_maxpool3x3s2, "af_relu_maxpool3x3s2"), (L.af_subsample2x, "af_subsample2x")):
        for args in ((None, 4096, 1, 8, 8, 64), (4096, None, 1, 8, 8, 64), (4096, 4096, 1, 8, 8, 12), (4096, 4096, 0, 8, 8, 64),
                     (4096, 4100, 1, 8, 8, 64), (4096, 4096, 4, 4096, 4096, 64)):
            assert fn(*args, None) == E and named(name), (name, args)
    for args in ((None, 4096, 4096, 1, 4, 4, 64), (4096, None, 4096, 1, 4, 4, 64), (4096, 4096, None, 1, 4, 4, 64),
                 (4096, 4096, 4096, 1, 4, 4, 20), (4096, 4096, 4096, 1, 0, 4, 64), (4096, 4096, 4096, 8, 2048, 2048, 64)):
        assert L.af_upsample2x_add(*args, None) == E and named("af_upsample2x_add"), args
    hw, st, ms = i6(8, 12, 4, 6, 2, 3), i3(8, 16, 32), f6(16, 32, 64, 128, 256, 512)
    dec = lambda h0=4096, h1=4096, h2=4096, hw=hw, st=st, ms=ms, B=2, cand=4096, count=4096, cap=1024: \
        L.af_retina_decode(h0, h1, h2, hw, st, ms, B, 0.5, cand, count, cap, None)
    for kw in (dict(h0=None), dict(h2=None), dict(hw=None), dict(st=None), dict(ms=None), dict(cand=None), dict(count=None), dict(B=0),
               dict(cap=1025), dict(cap=0), dict(hw=i6(8, 12, 4, 6, 0, 3)), dict(st=i3(8, 16, 0)), dict(ms=f6(16, 32, 64, 128, 256, 0)),
               dict(hw=i6(8192, 8192, 4, 6, 2, 3)), dict(hw=i6(2048, 2048, 2048, 2048, 4, 4), B=1), dict(cand=4104)):
        assert dec(**kw) == E and named("af_retina_decode"), kw
    nms = lambda cand=4096, count=4096, out=4096, oc=4096, B=2, cap=1024, max_det=64: L.af_retina_nms(cand, count, out, oc, B, cap, max_det, 0.4, None)
    for kw in (dict(cand=None), dict(count=None), dict(out=None), dict(oc=None), dict(B=0), dict(cap=1025), dict(cap=0), dict(max_det=0),
               dict(cap=512, max_det=513), dict(max_det=1025), dict(B=40000), dict(out=4104)):
        assert nms(**kw) == E and named("af_retina_nms"), kw


def test_planted_decode_inputs_meet_their_conditions():
    """The seeds of tests/test_hip_retinaface.py's decode + NMS cases, checked on the reference without a GPU: score and IoU margins, the
    tie, the suppression chain, and a kept count above max_det = 8 in the second case."""
    import test_hip_retinaface as G
    for case, (H, W, seed, max_det) in G.CASES.items():
        heads, sizes = G.planted_heads(H, W, seed)
        assert sum(2 * h.shape[1] for h in heads) == 252 and max(float((0.2 * h[..., :4]).abs().max()) for h in heads) <= 1.0
        n_full = G.check_input_conditions(heads, sizes, max_det, want_chain=True)
        assert n_full > 8, (case, n_full)
