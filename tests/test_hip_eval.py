"""The image-scoring encoders and evaluators on a real MI355X (`pytest -m gpu`): tiny configurations (width 128, 2 heads, 2 layers, image 32,
patch 8, projection 32) with weights rounded to fp16 on both sides, against the fp64 restatement of tests/vit_restatement.py (which
tests/test_eval_host.py pins to transformers).  Feature bound: rel-L2 < 5e-3, what tests/test_hip_clip.py holds the same layer class to.
Score bound: |delta| <= 1e-2, twice the feature bound -- a cosine of unit vectors moves by at most the sum of their relative errors."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vit_restatement as R

pytestmark = pytest.mark.gpu

FEAT_BOUND, SCORE_BOUND = 5e-3, 1e-2
TINY = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, patch_size=8, image_size=32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _seed_weights(model, seed):
    """Seeded parameters, rounded to fp16 (both sides then hold the same numbers); LayerNorm weights around 1."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            v = torch.randn(p.shape, generator=g) * 0.08
            if "norm" in n and n.endswith("weight"):
                v += 1.0
            p.copy_(v.half().float())
    return model.eval()


@pytest.fixture(scope="module")
def towers(dev):
    """(module on the device, its fp64 state dict) for the CLIP vision tower, the DINO tower and the CLIP text tower; built once."""
    from adaface_dev_amd.adaface.arc2face_models import clip_text_config
    from adaface_dev_amd.evaluation import vit
    out = {}
    for name, model in (("clip", vit.VisionTransformer(vit.clip_vision_config(projection_dim=32, **TINY))),
                        ("dino", vit.VisionTransformer(vit.dino_vit_config(**TINY)))):
        _seed_weights(model, {"clip": 11, "dino": 12}[name])
        out[name] = (model, R.to_dtype(model.state_dict()))
    tc = clip_text_config(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256, vocab_size=100, eos_token_id=99)
    tc.projection_dim = 32
    text = _seed_weights(vit.CLIPTextTower(tc), 13)
    out["text"] = (text, R.to_dtype(text.state_dict()))
    for k in out:
        out[k][0].to(dev)
    return out


def _images(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, s + (3,), generator=g, dtype=torch.int64).to(torch.uint8) for s in shapes]


def _ref_features(towers, name, images, patch_mask=None):
    """The restatement on a list of uint8 images (any sizes): (last hidden states, features), fp64."""
    model, sd = towers[name]
    c = model.config
    sc, sh = R.scale_shift(c.mean, c.std)
    pix = torch.cat([R.preprocess_ref(im[None], int(c.keep_aspect), c.image_size, c.image_size, {"bilinear": 0, "bicubic": 1}[c.filter], sc, sh)[0]
                     for im in images])
    return R.vision_forward(sd, c, pix, patch_mask)


@pytest.mark.parametrize("name", ["clip", "dino"])
def test_vision_tower_vs_restatement(dev, towers, name):
    model = towers[name][0]
    imgs = _images([(40, 52)] * 3, seed=21)
    feats, last = model.forward_u8(torch.stack(imgs).to(dev), return_hidden=True)
    torch.cuda.synchronize()
    ref_last, ref_feats = _ref_features(towers, name, imgs)
    e_last, e_feat = R.rel_l2(last.cpu(), ref_last), R.rel_l2(feats.cpu(), ref_feats)
    print(f"{name}: last hidden rel-L2 {e_last:.3e}, features {e_feat:.3e}")
    assert tuple(last.shape) == (3, 17, 128) and tuple(feats.shape) == (3, 32 if name == "clip" else 128)
    assert e_last < FEAT_BOUND and e_feat < FEAT_BOUND


def _ids():
    g = torch.Generator().manual_seed(22)
    ids = torch.randint(1, 98, (3, 77), generator=g)
    ids[:, 0] = 98
    for b, n in enumerate((6, 77, 30)):
        ids[b, n - 1:] = 99
    return ids


def test_text_tower_vs_restatement(dev, towers):
    text, sd = towers["text"]
    ids = _ids()
    feats, last = text.encode(ids.to(dev), return_hidden=True)
    torch.cuda.synchronize()
    ref_last, ref_feats = R.text_forward(sd, text.config, ids)
    e_last, e_feat = R.rel_l2(last.cpu(), ref_last), R.rel_l2(feats.cpu(), ref_feats)
    print(f"text: last hidden rel-L2 {e_last:.3e}, features {e_feat:.3e}")
    assert tuple(feats.shape) == (3, 32) and e_last < FEAT_BOUND and e_feat < FEAT_BOUND


@pytest.mark.parametrize("name", ["clip", "dino"])
def test_patch_mask(dev, towers, name):
    """Half the patches of batch item 1 hidden: the masked result is the masked restatement's, and it is not the unmasked one."""
    model = towers[name][0]
    imgs = _images([(40, 52)] * 3, seed=23)
    mask = torch.ones(3, 16, dtype=torch.bool)
    mask[1, ::2] = False
    x = torch.stack(imgs).to(dev)
    plain = model.forward_u8(x).cpu()
    masked = model.forward_u8(x, patch_mask=mask.to(dev)).cpu()
    ref_plain, ref_masked = _ref_features(towers, name, imgs)[1], _ref_features(towers, name, imgs, mask)[1]
    d_ref = R.rel_l2(ref_masked[1], ref_plain[1])
    print(f"{name}: masked vs restatement {R.rel_l2(masked, ref_masked):.3e}; masked vs unmasked, item 1: {R.rel_l2(masked[1], plain[1]):.3e} (restatement {d_ref:.3e})")
    assert d_ref > 4 * FEAT_BOUND, "the mask must move the reference well beyond the bound"
    assert R.rel_l2(masked, ref_masked) < FEAT_BOUND
    assert R.rel_l2(masked[1], plain[1]) > d_ref / 2
    assert R.rel_l2(masked[[0, 2]], plain[[0, 2]]) < FEAT_BOUND               # the other items see every patch
    with pytest.raises(ValueError, match="patch_mask"):
        model.forward_u8(x, patch_mask=mask[:, :8].to(dev))


class _TinyTokenizer:
    """The tokenizer protocol on a 100-word vocabulary: BOS 98, EOS = pad 99, words hashed into 1 .. 97."""

    def __call__(self, texts, padding="max_length", max_length=77, truncation=True, return_tensors="pt"):
        rows = []
        for t in texts:
            ids = [98] + [1 + zlib.crc32(w.encode()) % 97 for w in t.lower().split()][:max_length - 2] + [99]
            rows.append(ids + [99] * (max_length - len(ids)))
        return {"input_ids": torch.tensor(rows, dtype=torch.long)}


def _cos_mean(a, b):
    return float((F.normalize(a, dim=-1) @ F.normalize(b, dim=-1).T).mean())


def test_evaluators_vs_restatement(dev, towers):
    """Five seeded images of two sizes, interleaved: CLIP-I, CLIP-T and DINO scores against the restatement's, at max_batch 2 and 5."""
    from adaface_dev_amd.evaluation import eval_utils as EU
    imgs = _images([(40, 52), (36, 36), (40, 52), (36, 36), (40, 52)], seed=24)
    src, gen = imgs[:2], imgs[2:]
    prompt = "a photo of a z * person"
    tok = _TinyTokenizer()
    ids = tok([prompt.replace("*", "")])["input_ids"]
    text, tsd = towers["text"]
    ft = R.text_forward(tsd, text.config, ids)[1]
    want = {"clip_i": _cos_mean(_ref_features(towers, "clip", src)[1], _ref_features(towers, "clip", gen)[1]),
            "clip_t": _cos_mean(ft, _ref_features(towers, "clip", gen)[1]),
            "dino": _cos_mean(_ref_features(towers, "dino", src[:1])[1], _ref_features(towers, "dino", gen)[1])}
    got = {}
    for mb in (2, 5):
        ev = EU.ImageDirEvaluator(dev, clip_model=(towers["clip"][0], text), tokenizer=tok, max_batch=mb)
        dv = EU.ViTEvaluator(dev, dino_model=towers["dino"][0], max_batch=mb)
        sim_i, sim_t = ev.evaluate([g.numpy() for g in gen], [s.numpy() for s in src], prompt)
        got[mb] = {"clip_i": sim_i, "clip_t": sim_t, "dino": dv.img_to_img_similarity(torch.stack(src[:1]), gen)}      # (a uint8 tensor [1, H, W, 3])
        assert abs(ev.img_to_img_similarity(src, gen) - sim_i) < 1e-6 and abs(ev.txt_to_img_similarity(prompt.replace("*", ""), gen) - sim_t) < 1e-6
        f = ev.get_image_features(imgs)
        assert tuple(f.shape) == (5, 32) and torch.allclose(f.norm(dim=-1), torch.ones(5, device=dev), atol=1e-4)
        order = F.normalize(_ref_features(towers, "clip", imgs)[1], dim=-1)
        assert float((f.cpu().double() - order).norm(dim=-1).max()) < 2 * FEAT_BOUND, "features must come back in input order"
    print("want", want, "got", got)
    for k in want:
        assert abs(got[2][k] - want[k]) <= SCORE_BOUND and abs(got[5][k] - want[k]) <= SCORE_BOUND, (k, want[k], got)
        assert abs(got[2][k] - got[5][k]) <= SCORE_BOUND


def test_float_images_enter_quantised(dev, towers):
    """A float [B, 3, H, W] tensor in [-1, 1] gives what its quantised uint8 form gives, bit for bit."""
    from adaface_dev_amd.evaluation import eval_utils as EU
    dv = EU.ViTEvaluator(dev, dino_model=towers["dino"][0])
    x = torch.rand(2, 3, 36, 44, generator=torch.Generator().manual_seed(25)) * 2.4 - 1.2
    u8 = EU.float_images_to_u8(x)
    assert torch.equal(dv.get_image_features(x.to(dev)), dv.get_image_features(u8))


KPS = [[38.0, 40.0], [74.0, 41.0], [56.0, 60.0], [42.0, 80.0], [70.0, 81.0]]


def _photo(tag, seed):
    a = np.random.default_rng(seed).integers(0, 256, size=(96, 120, 3), dtype=np.uint8)
    a[0, 0, 0] = tag
    return a


def _stub_detector(img):
    """Fixed landmarks; tag 0 in the first pixel: nobody in the picture."""
    return [] if int(img[0, 0, 0]) == 0 else [(20.0, 20.0, 60.0, 70.0, 0.9, KPS)]


def test_face_similarity(dev, tmp_path):
    from PIL import Image
    from adaface_dev_amd.adaface.face_align import FaceIDExtractor
    from adaface_dev_amd.evaluation import eval_utils as EU
    proj = torch.randn(14 * 14 * 3, 512, generator=torch.Generator().manual_seed(26)).to(dev)

    def recogniser(crops):                                   # a stand-in on the aligned crops fp16 [N, 112, 112, 8] -> [N, 512]
        return crops[:, ::8, ::8, :3].float().reshape(crops.shape[0], -1) @ proj

    ex = FaceIDExtractor(recogniser, _stub_detector, device=dev)
    ev = EU.FaceSimilarityEvaluator(ex)
    a, b, nobody = _photo(1, 31), _photo(2, 32), _photo(0, 33)
    sim, faceless = ev.compare([a, a], [a, a])
    assert abs(sim - 1.0) < 1e-3 and faceless == (0, 0)
    sim_ab, faceless = ev.compare([a, nobody], [b])
    assert faceless == (1, 0) and -1.0 <= sim_ab < 0.999
    _, ia = ex.extract([a])
    _, ib = ex.extract([b])
    assert abs(sim_ab - float(ia[0] @ ib[0])) < 1e-5
    assert ev.compare([nobody, nobody], [a]) == (0.0, (2, 0))
    assert ev.compare([a], [nobody]) == (0.0, (0, 1))
    for d in ("one", "two"):
        (tmp_path / d).mkdir()
        for i in range(2):
            Image.fromarray(a).save(tmp_path / d / f"{i}.png")
    sim, faceless = EU.compare_face_folders(str(tmp_path / "one"), str(tmp_path / "two"), ex)
    assert abs(sim - 1.0) < 1e-3 and faceless == (0, 0)
