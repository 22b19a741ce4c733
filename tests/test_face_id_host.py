"""Face IDs from images, the host side (no GPU): the 5-point similarity (`adaface/face_align.py::estimate_similarity`), IResNet's module tree
and checkpoint naming (`adaface/iresnet.py`), `FaceIDExtractor`'s bookkeeping with a stub detector / crop / recogniser, and the route from
`image_paths` to the extractor through `Arc2Face_ID2AdaPrompt` (INTEGRATION.md "Face IDs from images").  The kernels and the network's
arithmetic are pinned on the GPU in tests/test_hip_face_id.py."""
import numpy as np
import pytest
import torch

from standin import StandInCLIP


def _similarity(scale, deg, shift):
    a = np.deg2rad(deg)
    return np.array([[scale * np.cos(a), -scale * np.sin(a), shift[0]], [scale * np.sin(a), scale * np.cos(a), shift[1]]])


def _apply(m, pts):
    return np.asarray(pts, dtype=np.float64) @ m[:, :2].T + m[:, 2]


def _compose(a, b):
    """2 x 3 matrix of x -> a(b(x))."""
    return np.concatenate([a[:, :2] @ b[:, :2], (a[:, :2] @ b[:, 2] + a[:, 2])[:, None]], axis=1)


def test_template_is_insightface_arcface_dst():
    from adaface_dev_amd.adaface.face_align import ARCFACE_TEMPLATE_112 as T
    assert T.dtype == np.float64 and T.tolist() == [[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655],
                                                    [70.7299, 92.2041]]


def test_estimate_similarity_identity_known_transform_and_mirror():
    from adaface_dev_amd.adaface.face_align import ARCFACE_TEMPLATE_112 as T, estimate_similarity
    eye = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    fwd, inv = estimate_similarity(T)
    assert np.abs(fwd - eye).max() < 1e-9 and np.abs(inv - eye).max() < 1e-9
    # landmarks = S(template) with a known similarity S: the estimate is S^-1 (image -> crop), its inverse S
    S = _similarity(2.3, 17.0, (40.0, -25.0))
    fwd, inv = estimate_similarity(_apply(S, T))
    assert np.abs(inv - S).max() < 1e-9
    assert np.abs(_apply(fwd, _apply(S, T)) - T).max() < 1e-9
    assert np.abs(_compose(fwd, inv) - eye).max() < 1e-9 and np.abs(_compose(inv, fwd) - eye).max() < 1e-9
    assert abs(np.linalg.det(fwd[:, :2]) - 1 / 2.3 ** 2) < 1e-9
    # horizontally mirrored landmarks (a flipped photo whose detector kept the left / right labels): still a proper similarity
    mirrored = _apply(S, T) * np.array([-1.0, 1.0]) + np.array([300.0, 0.0])
    fwd, inv = estimate_similarity(mirrored)
    assert np.linalg.det(fwd[:, :2]) > 0 and np.linalg.det(inv[:, :2]) > 0
    assert np.abs(_compose(fwd, inv) - eye).max() < 1e-9
    r = fwd[:, :2] / np.sqrt(np.linalg.det(fwd[:, :2]))
    assert np.abs(r @ r.T - np.eye(2)).max() < 1e-9                       # rotation times scale, nothing else
    with pytest.raises(ValueError):
        estimate_similarity(np.zeros((5, 2)))


def _expected_keys(depths):
    bn = lambda p: [f"{p}.{s}" for s in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    keys = ["conv1.weight"] + bn("bn1") + ["prelu.weight"]
    for li, n in enumerate(depths, start=1):
        for bi in range(n):
            p = f"layer{li}.{bi}"
            keys += bn(f"{p}.bn1") + [f"{p}.conv1.weight"] + bn(f"{p}.bn2") + [f"{p}.prelu.weight", f"{p}.conv2.weight"] + bn(f"{p}.bn3")
            if bi == 0:
                keys += [f"{p}.downsample.0.weight"] + bn(f"{p}.downsample.1")
    return keys + bn("bn2") + ["fc.weight", "fc.bias"] + bn("features")


@pytest.mark.parametrize("factory,depths", [("iresnet100", (3, 13, 30, 3)), ("iresnet50", (3, 4, 14, 3))])
def test_iresnet_state_dict_follows_arcface_torch_naming(factory, depths):
    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface import iresnet
    with rng.skip_default_init():
        m = getattr(iresnet, factory)()
    sd = m.state_dict()
    assert sorted(sd) == sorted(_expected_keys(depths))
    assert tuple(len(layer) for layer in (m.layer1, m.layer2, m.layer3, m.layer4)) == depths
    widths = (64, 128, 256, 512)
    for li, w in enumerate(widths, start=1):
        layer = getattr(m, f"layer{li}")
        cin = 64 if li == 1 else widths[li - 2]
        assert tuple(sd[f"layer{li}.0.conv1.weight"].shape) == (w, cin, 3, 3) and tuple(sd[f"layer{li}.0.downsample.0.weight"].shape) == (w, cin, 1, 1)
        assert [b.stride for b in layer] == [2] + [1] * (len(layer) - 1)
        assert all(b.downsample is None for b in layer[1:]) and all(tuple(b.prelu.weight.shape) == (w,) for b in layer)
    assert tuple(sd["conv1.weight"].shape) == (64, 3, 3, 3) and tuple(sd["prelu.weight"].shape) == (64,)
    assert tuple(sd["fc.weight"].shape) == (512, 512 * 7 * 7) and tuple(sd["features.weight"].shape) == (512,)
    # a checkpoint of that family (num_batches_tracked buffers included) loads strictly
    foreign = {k: torch.full_like(v, 3) for k, v in sd.items()}
    with rng.skip_default_init():
        m2 = getattr(iresnet, factory)()
    m2.load_state_dict(foreign, strict=True)
    assert all(torch.equal(v, foreign[k]) for k, v in m2.state_dict().items())
    assert m2.inference_only is True


def test_iresnet_reduced_depths_and_training_mode_raises():
    from adaface_dev_amd.adaface.iresnet import IResNet
    m = IResNet(layers=(2, 1, 1, 1))
    assert sorted(m.state_dict()) == sorted(_expected_keys((2, 1, 1, 1)))
    m.train()
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 3, 112, 112))
    with pytest.raises(RuntimeError, match="CPU"):                     # no CPU fallback
        m.eval()(torch.zeros(1, 3, 112, 112))


# ---- FaceIDExtractor with stubs: a detector keyed by the image's first pixel, a crop that records its arguments, a CPU recogniser ------
KPS_A = [[30.0, 40.0], [70.0, 41.0], [50.0, 60.0], [35.0, 80.0], [66.0, 81.0]]
KPS_B = [[130.0, 90.0], [190.0, 95.0], [160.0, 130.0], [135.0, 160.0], [185.0, 163.0]]


def _img(tag, h=96, w=120):
    a = np.full((h, w, 3), 17, dtype=np.uint8)
    a[0, 0, 0] = tag
    return a


def _detector(img):
    tag = int(img[0, 0, 0])
    if tag == 0:
        return []
    small, large = (5.0, 5.0, 20.0, 20.0, 0.99, KPS_A), (40.0, 30.0, 30.0 + tag, 40.0, 0.50, KPS_B)       # the larger box wins, not the surer
    return [small, large] if tag % 2 else [large, small]


@pytest.fixture
def stub_extractor(monkeypatch):
    from adaface_dev_amd import ops
    from adaface_dev_amd.adaface.face_align import FaceIDExtractor
    calls = []

    def crop(image_u8, inv_mats, size=112):
        assert image_u8.dtype == torch.uint8 and image_u8.dim() == 3 and inv_mats.dtype == torch.float32 and tuple(inv_mats.shape) == (1, 2, 3)
        calls.append((image_u8.clone(), inv_mats.clone(), size))
        out = torch.zeros((1, size, size, 8), dtype=torch.float16)
        out[..., 0] = float(image_u8[0, 0, 0]) / 8
        return out

    def recogniser(crops):
        assert crops.dtype == torch.float16 and tuple(crops.shape[1:]) == (112, 112, 8)
        t = crops[:, 0, 0, 0].float()
        return torch.stack([t, 2 * torch.ones_like(t)] + [torch.zeros_like(t)] * 510, dim=1).half()

    monkeypatch.setattr(ops, "face_align_crop", crop)
    return FaceIDExtractor(recogniser, _detector, device="cpu"), calls


def test_extractor_takes_the_largest_face_and_counts_faceless_images(stub_extractor):
    from adaface_dev_amd.adaface.face_align import estimate_similarity
    ex, calls = stub_extractor
    faceless, ids = ex.extract([_img(3), _img(0), _img(8)])
    assert faceless == 1 and tuple(ids.shape) == (2, 512) and ids.dtype == torch.float32
    assert len(calls) == 2 and [int(c[0][0, 0, 0]) for c in calls] == [3, 8] and all(c[2] == 112 for c in calls)
    want = torch.from_numpy(estimate_similarity(KPS_B)[1].astype(np.float32))[None]                  # the LARGE face, in either list order
    assert all(torch.equal(c[1], want) for c in calls)
    assert tuple(calls[0][0].shape) == (96, 120, 3)                                                   # uploaded as it is: not resized
    e = torch.tensor([[3 / 8, 2.0], [1.0, 2.0]])
    assert torch.allclose(ids[:, :2], e / e.norm(dim=1, keepdim=True), atol=1e-6) and torch.allclose(ids.norm(dim=1), torch.ones(2), atol=1e-6)
    _, avg = ex.extract([_img(3), _img(0), _img(8)], calc_avg=True)
    assert tuple(avg.shape) == (1, 512) and torch.equal(avg, torch.nn.functional.normalize(ids.mean(dim=0, keepdim=True), dim=-1))


def test_extractor_skips_or_raises_without_a_face_and_returns_none_when_all_are_faceless(stub_extractor, tmp_path):
    from PIL import Image
    ex, calls = stub_extractor
    assert ex.extract([_img(0), _img(0)]) == (2, None) and not calls
    with pytest.raises(ValueError, match="image #1"):
        ex.extract([_img(3), _img(0)], skip_non_faces=False)
    path = str(tmp_path / "nobody.png")
    Image.fromarray(_img(0)).save(path)
    with pytest.raises(ValueError, match="nobody.png"):
        ex.extract([path], skip_non_faces=False)
    # paths and PIL images (any mode) are read as RGB
    p5 = str(tmp_path / "five.png")
    Image.fromarray(_img(5)).save(p5)
    faceless, ids = ex.extract([p5, Image.fromarray(_img(5)), Image.fromarray(_img(5)).convert("RGBA")])
    assert faceless == 0 and tuple(ids.shape) == (3, 512) and torch.equal(ids[0], ids[1]) and torch.equal(ids[0], ids[2])
    with pytest.raises(ValueError):
        ex.extract([np.zeros((8, 8, 3), dtype=np.float32)])


# ---- the route from images to the extractor -----------------------------------------------------------------------------------------
def _id2ada(extractor=None):
    from adaface_dev_amd.adaface.arc2face_models import clip_text_config
    from adaface_dev_amd.adaface.face_id_to_ada_prompt import Arc2Face_ID2AdaPrompt
    from adaface_dev_amd.adaface.subj_basis_generator import SubjBasisGenerator
    cc = clip_text_config(hidden_size=64, num_attention_heads=2, num_hidden_layers=1, intermediate_size=64)
    g = SubjBasisGenerator(dtype=torch.float32, num_id_vecs=16, num_static_img_suffix_embs=0, output_dim=768, clip_config=cc)
    g.prompt2token_proj = StandInCLIP(768, seed=73)
    a = Arc2Face_ID2AdaPrompt(clip_config=cc, subj_basis_generator=g, text_to_image_prompt_encoder=StandInCLIP(768, seed=75),
                              face_id_extractor=extractor)
    a.__class__.dtype = property(lambda self: torch.float32)
    return a


def test_unconfigured_image_paths_raise_the_same_not_implemented_error():
    a = _id2ada()
    assert a.face_id_extractor is None
    for kw in (dict(image_paths=["a.png"]), dict(image_objs=[_img(3)])):
        with pytest.raises(NotImplementedError) as e:
            a.get_img_prompt_embs(None, **kw)
        assert str(e.value) == "face detection / ID extraction from images uses insightface ONNX (third-party, absent)"
    with pytest.raises(NotImplementedError):
        a.generate_adaface_embeddings(image_paths=["a.png"])


def test_image_paths_reach_the_extractor_and_continue_on_the_id_path(stub_extractor):
    from adaface_dev_amd import rng
    ex, calls = stub_extractor
    a = _id2ada(ex)
    imgs = [_img(3), _img(0), _img(8)]
    for avg in ("id_emb", None, "img_prompt_emb"):
        ids = ex.extract(imgs, calc_avg=(avg == "id_emb"))[1]
        with torch.no_grad():
            n, fid, pos, neg = a.get_img_prompt_embs(None, image_paths=imgs, avg_at_stage=avg)
            n0, fid0, pos0, _ = a.get_img_prompt_embs(ids, avg_at_stage=avg)
            n2, fid2, _, _ = a.get_img_prompt_embs(None, image_objs=imgs, avg_at_stage=avg)
            embs, ip, lens = a.generate_adaface_embeddings(image_paths=imgs, avg_at_stage=avg)
            embs0, ip0, lens0 = a.generate_adaface_embeddings(face_id_embs=ids, avg_at_stage=avg)
        assert (n, n0, n2) == (1, 0, 1) and neg is None
        assert torch.equal(fid, fid0) and torch.equal(pos, pos0) and torch.equal(fid2, fid0)
        assert torch.equal(embs, embs0) and torch.equal(ip, ip0) and lens == lens0
    with torch.no_grad():
        assert a.get_img_prompt_embs(None, image_paths=[_img(0), _img(0)]) == (2, None, None, None)
        assert a.generate_adaface_embeddings(image_paths=[_img(0)]) == (None, None, [16])
        with pytest.raises(ValueError):
            a.get_img_prompt_embs(None, image_paths=[_img(0)], skip_non_faces=False)
        # IDs handed in together with images win: the extractor is not asked
        calls.clear()
        given = torch.nn.functional.normalize(rng.synth_input("fid.given", (1, 512), seed=3), dim=-1)
        e1 = a.generate_adaface_embeddings(image_paths=imgs, face_id_embs=given)[0]
        assert not calls and torch.equal(e1, a.generate_adaface_embeddings(face_id_embs=given)[0])


def test_wrapper_hands_the_extractor_to_the_encoder_it_builds():
    from adaface_dev_amd import TINY_UNET_CONFIG
    from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper
    from adaface_dev_amd.adaface.arc2face_models import clip_text_config
    cc = clip_text_config(hidden_size=64, num_attention_heads=1, num_hidden_layers=1, intermediate_size=128)
    marker = object()
    w = AdaFaceWrapper(pipeline_name=None, clip_config=cc, unet_config=dict(TINY_UNET_CONFIG), device="cpu", face_id_extractor=marker)
    assert w.id2ada_prompt_encoder.face_id_extractor is marker
    w = AdaFaceWrapper(pipeline_name=None, clip_config=cc, unet_config=dict(TINY_UNET_CONFIG), device="cpu")
    assert w.id2ada_prompt_encoder.face_id_extractor is None


def test_c_abi_refuses_bad_crop_arguments_before_any_launch():
    """Argument validation precedes the launch, so it is observable without a GPU (the pointers are never dereferenced)."""
    from adaface_dev_amd import _lib
    L = _lib.lib()
    crop = lambda H, W, F, size, img=4096, out=4096: L.af_face_align_crop(img, 4096, out, H, W, F, size, None)
    for args in ((32768, 32768, 1, 112), (37, 53, 0, 112), (37, 53, -1, 112), (37, 53, 1, 96), (37, 53, 1, 0), (0, 53, 1, 112)):
        assert crop(*args) == _lib.AF_E_BADARG and b"af_face_align_crop" in L.af_last_error(), args
    assert crop(37, 53, 1, 112, img=None) == _lib.AF_E_BADARG and crop(37, 53, 1, 112, out=4100) == _lib.AF_E_BADARG
    assert L.af_affine_prelu_ch(4096, None, None, None, 4096, 5, 12, None) == _lib.AF_E_BADARG
    assert L.af_affine_prelu_ch(4096, 4096, None, None, 4096, 5, 8, None) == _lib.AF_E_BADARG
