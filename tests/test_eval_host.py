"""Image scoring without a GPU (INTEGRATION.md "Scoring images"): the fp64 restatements of tests/vit_restatement.py against randomly
initialised ``transformers`` models, the two checkpoint layouts of each loader, the resize geometry, the evaluators' arithmetic on injected
feature functions, and af_vit_patch_rows' argument checks (they precede any launch, so they are observable here)."""
import ctypes

import numpy as np
import pytest
import torch

import vit_restatement as R
from adaface_dev_amd import _lib, ops
from adaface_dev_amd.adaface.face_align import load_rgb_u8
from adaface_dev_amd.evaluation import eval_utils as EU
from adaface_dev_amd.evaluation import vit

transformers = pytest.importorskip("transformers")

TINY = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2)


def _randomise(model, seed):
    """Every parameter seeded and away from its initial value (zero biases and unit LayerNorm weights would hide a swapped pair)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.08)
            if "norm" in n and n.endswith("weight") and p.dim() == 1:
                p.add_(1.0)
    return model.eval()


@pytest.fixture(scope="module")
def hf_clip_vision():
    c = transformers.CLIPVisionConfig(image_size=32, patch_size=8, projection_dim=32, hidden_act="quick_gelu", layer_norm_eps=1e-5,
                                      attn_implementation="eager", **TINY)
    return _randomise(transformers.CLIPVisionModelWithProjection(c), 1)


@pytest.fixture(scope="module")
def hf_clip_text():
    c = transformers.CLIPTextConfig(vocab_size=100, max_position_embeddings=16, projection_dim=32, hidden_act="quick_gelu", layer_norm_eps=1e-5,
                                    bos_token_id=98, eos_token_id=99, pad_token_id=99, attn_implementation="eager", **TINY)
    return _randomise(transformers.CLIPTextModelWithProjection(c), 2)


@pytest.fixture(scope="module")
def hf_dino():
    c = transformers.ViTConfig(image_size=32, patch_size=8, hidden_act="gelu", layer_norm_eps=1e-12, qkv_bias=True, attn_implementation="eager",
                               **TINY)
    return _randomise(transformers.ViTModel(c, add_pooling_layer=False), 3)


def _clip_sd(hf_clip_vision, hf_clip_text):
    return {**hf_clip_vision.state_dict(), **hf_clip_text.state_dict()}


def _pix(seed=5, B=3):
    return torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(seed))


def _ids(seed=6, B=3, T=16):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 98, (B, T), generator=g)
    ids[:, 0] = 98
    for b, n in enumerate((5, 16, 9)[:B]):                 # EOS at different positions, padded with EOS as CLIP's tokenizer does
        ids[b, n - 1:] = 99
    return ids


# ---- (a) the restatement against transformers, fp32 vs fp64 of the same arithmetic -------------------------------------------------------------
def test_restatement_matches_transformers_clip_vision(hf_clip_vision, hf_clip_text):
    vision, _ = vit.load_clip(_clip_sd(hf_clip_vision, hf_clip_text))
    assert (vision.config.hidden_size, vision.config.num_hidden_layers, vision.config.num_attention_heads) == (128, 2, 2)
    assert (vision.config.patch_size, vision.config.image_size, vision.config.projection_dim, vision.config.intermediate_size) == (8, 32, 32, 256)
    pix = _pix()
    with torch.no_grad():
        out = hf_clip_vision(pixel_values=pix)
    last, feats = R.vision_forward(R.to_dtype(vision.state_dict()), vision.config, pix.double())
    assert R.rel_l2(out.last_hidden_state, last) <= 1e-4
    assert R.rel_l2(out.image_embeds, feats) <= 1e-4


def test_restatement_matches_transformers_dino(hf_dino):
    model = vit.load_dino(hf_dino.state_dict())
    c = model.config
    assert (c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.patch_size, c.image_size, c.projection_dim) == (128, 2, 2, 8, 32, 0)
    assert c.hidden_act == "gelu" and c.layer_norm_eps == 1e-12 and model.patch_embedding.bias is not None and model.pre_layrnorm is None
    pix = _pix(7)
    with torch.no_grad():
        out = hf_dino(pixel_values=pix)
    last, feats = R.vision_forward(R.to_dtype(model.state_dict()), c, pix.double())
    assert R.rel_l2(out.last_hidden_state, last) <= 1e-4
    assert torch.equal(feats, last[:, 0])


def test_restatement_matches_transformers_clip_text(hf_clip_vision, hf_clip_text):
    _, text = vit.load_clip(_clip_sd(hf_clip_vision, hf_clip_text))
    assert (text.config.hidden_size, text.config.vocab_size, text.config.max_position_embeddings, text.config.eos_token_id) == (128, 100, 16, 99)
    ids = _ids()
    with torch.no_grad():
        out = hf_clip_text(input_ids=ids)
    last, feats = R.text_forward(R.to_dtype(text.state_dict()), text.config, ids)
    assert R.rel_l2(out.last_hidden_state, last) <= 1e-4
    assert R.rel_l2(out.text_embeds, feats) <= 1e-4


def test_masked_restatement_differs_and_ignores_hidden_patches(hf_clip_vision, hf_clip_text):
    """The patch mask of the restatement itself: hiding patches changes the result, and what the hidden patches hold no longer matters
    to the CLS feature."""
    vision, _ = vit.load_clip(_clip_sd(hf_clip_vision, hf_clip_text))
    sd, pix = R.to_dtype(vision.state_dict()), _pix().double()
    mask = torch.ones(3, 16, dtype=torch.bool)
    mask[1, ::2] = False
    f0 = R.vision_forward(sd, vision.config, pix)[1]
    f1 = R.vision_forward(sd, vision.config, pix, mask)[1]
    assert R.rel_l2(f1[1], f0[1]) > 1e-3 and torch.allclose(f1[0], f0[0], rtol=0, atol=1e-12)
    pix2 = pix.clone()
    pix2[1, :, 0:8, 0:8] += 1.0                                 # patch 0 of item 1 is hidden
    f2 = R.vision_forward(sd, vision.config, pix2, mask)[1]
    assert torch.allclose(f2, f1, rtol=0, atol=1e-12)


# ---- (b) the second layout of each loader, built here from the transformers state dict ---------------------------------------------------------
def _openai_layers(sd, src, dst, out):
    n = 0
    while f"{src}{n}.layer_norm1.weight" in sd:
        s, d = f"{src}{n}.", f"{dst}{n}."
        for t in ("weight", "bias"):
            out[d + "attn.in_proj_" + t] = torch.cat([sd[s + f"self_attn.{x}_proj.{t}"] for x in "qkv"], dim=0)
            out[d + "attn.out_proj." + t] = sd[s + "self_attn.out_proj." + t]
            out[d + "ln_1." + t], out[d + "ln_2." + t] = sd[s + "layer_norm1." + t], sd[s + "layer_norm2." + t]
            out[d + "mlp.c_fc." + t], out[d + "mlp.c_proj." + t] = sd[s + "mlp.fc1." + t], sd[s + "mlp.fc2." + t]
        n += 1
    assert n == 2


def openai_layout(sd):
    v, t = "vision_model.", "text_model."
    out = {"visual.class_embedding": sd[v + "embeddings.class_embedding"], "visual.positional_embedding": sd[v + "embeddings.position_embedding.weight"],
           "visual.conv1.weight": sd[v + "embeddings.patch_embedding.weight"], "visual.proj": sd["visual_projection.weight"].t().contiguous(),
           "positional_embedding": sd[t + "embeddings.position_embedding.weight"], "token_embedding.weight": sd[t + "embeddings.token_embedding.weight"],
           "text_projection": sd["text_projection.weight"].t().contiguous(), "logit_scale": torch.tensor(4.6),
           "input_resolution": torch.tensor(32), "context_length": torch.tensor(16), "vocab_size": torch.tensor(100)}
    for a, b in (("ln_pre", "pre_layrnorm"), ("ln_post", "post_layernorm")):
        for x in ("weight", "bias"):
            out[f"visual.{a}.{x}"] = sd[f"{v}{b}.{x}"]
    for x in ("weight", "bias"):
        out["ln_final." + x] = sd[t + "final_layer_norm." + x]
    _openai_layers(sd, v + "encoder.layers.", "visual.transformer.resblocks.", out)
    _openai_layers(sd, t + "encoder.layers.", "transformer.resblocks.", out)
    return out


def dino_hf4_layout(sd):
    """The ViTModel layout of the published facebook/dino-vits16 files (transformers 4 names), from whatever the installed transformers saves."""
    if any(k.startswith("encoder.layer.") for k in sd):
        return dict(sd)
    ren = (("attention.q_proj.", "attention.attention.query."), ("attention.k_proj.", "attention.attention.key."),
           ("attention.v_proj.", "attention.attention.value."), ("attention.o_proj.", "attention.output.dense."),
           ("mlp.fc1.", "intermediate.dense."), ("mlp.fc2.", "output.dense."))
    out = {}
    for k, v in sd.items():
        if k.startswith("layers."):
            n, _, tail = k[len("layers."):].partition(".")
            for a, b in ren:
                if tail.startswith(a):
                    tail = b + tail[len(a):]
                    break
            k = f"encoder.layer.{n}.{tail}"
        out[k] = v
    return out


def dino_fb_layout(sd):
    sd = dino_hf4_layout(sd)
    e = "embeddings."
    out = {"cls_token": sd[e + "cls_token"], "pos_embed": sd[e + "position_embeddings"], "patch_embed.proj.weight": sd[e + "patch_embeddings.projection.weight"],
           "patch_embed.proj.bias": sd[e + "patch_embeddings.projection.bias"], "norm.weight": sd["layernorm.weight"], "norm.bias": sd["layernorm.bias"]}
    n = 0
    while f"encoder.layer.{n}.layernorm_before.weight" in sd:
        s, d = f"encoder.layer.{n}.", f"blocks.{n}."
        for t in ("weight", "bias"):
            out[d + "attn.qkv." + t] = torch.cat([sd[s + f"attention.attention.{x}.{t}"] for x in ("query", "key", "value")], dim=0)
            out[d + "attn.proj." + t] = sd[s + "attention.output.dense." + t]
            out[d + "norm1." + t], out[d + "norm2." + t] = sd[s + "layernorm_before." + t], sd[s + "layernorm_after." + t]
            out[d + "mlp.fc1." + t], out[d + "mlp.fc2." + t] = sd[s + "intermediate.dense." + t], sd[s + "output.dense." + t]
        n += 1
    assert n == 2
    return out


def _same_parameters(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_both_clip_layouts_load_identically(hf_clip_vision, hf_clip_text):
    sd = _clip_sd(hf_clip_vision, hf_clip_text)
    v1, t1 = vit.load_clip(sd)
    v2, t2 = vit.load_clip(openai_layout(sd))
    _same_parameters(v1, v2)
    _same_parameters(t1, t2)
    assert vars(v1.config) == vars(v2.config) and vars(t1.config) == vars(t2.config)
    assert not any(torch.equal(p, torch.zeros_like(p)) for p in v1.parameters())
    # position_ids buffers (older transformers checkpoints carry them) are ignored
    vit.load_clip({**sd, "vision_model.embeddings.position_ids": torch.arange(17)[None], "text_model.embeddings.position_ids": torch.arange(16)[None]})


def test_both_dino_layouts_load_identically(hf_dino):
    sd = hf_dino.state_dict()
    m1 = vit.load_dino(sd)
    m2 = vit.load_dino(dino_fb_layout(sd))
    m3 = vit.load_dino(dino_hf4_layout(sd))
    assert "encoder.layer.1.attention.attention.query.weight" in dino_hf4_layout(sd) and "blocks.1.attn.qkv.weight" in dino_fb_layout(sd)
    _same_parameters(m1, m2)
    _same_parameters(m1, m3)
    assert vars(m1.config) == vars(m2.config) == vars(m3.config)
    vit.load_dino({**dino_hf4_layout(sd), "pooler.dense.weight": torch.zeros(128, 128), "pooler.dense.bias": torch.zeros(128)})


@pytest.mark.parametrize("layout", ["hf", "openai"])
def test_clip_loader_is_strict(hf_clip_vision, hf_clip_text, layout):
    sd = _clip_sd(hf_clip_vision, hf_clip_text)
    if layout == "openai":
        sd = openai_layout(sd)
        gone, extra, bad = "visual.transformer.resblocks.1.mlp.c_fc.bias", "visual.transformer.resblocks.1.mlp.c_fc.gamma", "transformer.resblocks.0.ln_2.weight"
        gone_named, bad_named = "layers.1.mlp.fc1.bias", "text_model.encoder.layers.0.layer_norm2.weight"
    else:
        gone, extra, bad = "vision_model.encoder.layers.1.mlp.fc1.bias", "vision_model.encoder.layers.1.mlp.fc1.gamma", "text_model.encoder.layers.0.layer_norm2.weight"
        gone_named, bad_named = "layers.1.mlp.fc1.bias", bad
    with pytest.raises(ValueError, match="missing.*" + gone_named.replace(".", r"\.")):
        vit.load_clip({k: v for k, v in sd.items() if k != gone})
    with pytest.raises(ValueError, match=r"unexpected.*mlp\.(c_fc|fc1)\.gamma"):
        vit.load_clip({**sd, extra: torch.zeros(3)})
    with pytest.raises(ValueError, match="wrong shape.*" + bad_named.replace(".", r"\.")):
        vit.load_clip({**sd, bad: torch.zeros(127)})


@pytest.mark.parametrize("layout", ["hf", "fb"])
def test_dino_loader_is_strict(hf_dino, layout):
    sd = dino_hf4_layout(hf_dino.state_dict())
    if layout == "fb":
        sd = dino_fb_layout(sd)
        gone, bad = "blocks.1.attn.proj.bias", "norm.weight"
    else:
        gone, bad = "encoder.layer.1.attention.output.dense.bias", "layernorm.weight"
    with pytest.raises(ValueError, match=r"missing.*layers\.1\.self_attn\.out_proj\.bias"):
        vit.load_dino({k: v for k, v in sd.items() if k != gone})
    with pytest.raises(ValueError, match=r"unexpected.*register_tokens"):
        vit.load_dino({**sd, "register_tokens": torch.zeros(1, 4, 128)})
    with pytest.raises(ValueError, match=r"wrong shape.*post_layernorm\.weight"):
        vit.load_dino({**sd, bad: torch.zeros(127)})


def test_presets():
    b, l, d = vit.clip_vision_config(), vit.clip_vision_config("ViT-L/14"), vit.dino_vit_config()
    assert (b.hidden_size, b.num_hidden_layers, b.num_attention_heads, b.patch_size, b.image_size, b.projection_dim) == (768, 12, 12, 32, 224, 512)
    assert (l.hidden_size, l.num_hidden_layers, l.num_attention_heads, l.patch_size, l.image_size, l.projection_dim) == (1024, 24, 16, 14, 224, 768)
    assert (d.hidden_size, d.num_hidden_layers, d.num_attention_heads, d.patch_size, d.image_size, d.projection_dim) == (384, 12, 6, 16, 224, 0)
    assert (b.hidden_act, b.layer_norm_eps, b.pre_layernorm, b.patch_bias) == ("quick_gelu", 1e-5, True, False)
    assert (d.hidden_act, d.layer_norm_eps, d.pre_layernorm, d.patch_bias) == ("gelu", 1e-12, False, True)
    t = vit.clip_text_tower_config()
    assert (t.hidden_size, t.num_attention_heads, t.intermediate_size, t.projection_dim, t.max_position_embeddings) == (512, 8, 2048, 512, 77)
    m = vit.VisionTransformer(vit.clip_vision_config(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, patch_size=14, image_size=28, projection_dim=16))
    assert m.patch_kcols() == 640 and m.num_patches == 4 and m.feature_dim == 16
    with pytest.raises(RuntimeError, match="no CPU"):
        m.forward_rows(torch.zeros(4, 640), 1)


# ---- (c) resize geometry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", [ops.vit_resize_geometry, R.resize_geometry], ids=["package", "restatement"])
def test_resize_geometry(geometry):
    assert geometry(96, 130, True, 32, 32) == (32, 43, 0, 6)          # 5.5 -> 6
    assert geometry(39, 50, True, 32, 32) == (32, 41, 0, 4)           # 4.5 -> 4
    assert geometry(64, 48, True, 32, 32) == (42, 32, 5, 0)           # portrait
    assert geometry(300, 70, True, 28, 28) == (120, 28, 46, 0)
    assert geometry(450, 41, False, 999, 32) == (32, 32, 0, 0)
    assert geometry(512, 512, True, 224, 224) == (224, 224, 0, 0)


# ---- (d) evaluator arithmetic on injected feature functions ---------------------------------------------------------------------------------
class _Vision:
    """features = (mean of channel 0, mean of channel 1, H, W): distinguishes the images and records the batches it was called with."""

    def __init__(self):
        self.calls = []

    def forward_u8(self, batch):
        assert batch.dtype == torch.uint8 and batch.dim() == 4 and batch.shape[3] == 3
        self.calls.append(tuple(batch.shape))
        m = batch.float().mean(dim=(1, 2))
        hw = torch.tensor([batch.shape[1], batch.shape[2]], dtype=torch.float32).expand(batch.shape[0], 2)
        return torch.cat([m[:, :2], hw], dim=1)


class _Text:
    def __init__(self):
        self.seen = []

    def encode(self, ids):
        return torch.tensor([[1.0, 2.0, 0.0, 0.0]]).expand(ids.shape[0], 4)


class _Tok:
    def __init__(self):
        self.texts = []

    def __call__(self, texts, **kw):
        assert kw["max_length"] == 77 and kw["padding"] == "max_length"
        self.texts.append(list(texts))
        return {"input_ids": torch.zeros((len(texts), 77), dtype=torch.long)}


def _images():
    g = torch.Generator().manual_seed(0)
    return [torch.randint(0, 256, s + (3,), generator=g, dtype=torch.int64).to(torch.uint8).numpy() for s in ((8, 12), (6, 6), (8, 12), (6, 6), (8, 12))]


def test_size_grouping_keeps_input_order():
    ims, v = _images(), _Vision()
    f = EU.encode_grouped(ims, v.forward_u8, "cpu", max_batch=2)
    assert v.calls == [(2, 8, 12, 3), (1, 8, 12, 3), (2, 6, 6, 3)]
    want = torch.stack([torch.tensor([im[..., 0].mean(), im[..., 1].mean(), im.shape[0], im.shape[1]], dtype=torch.float32) for im in ims])
    assert torch.allclose(f, want, atol=1e-4)
    assert EU.size_groups([(8, 12), (6, 6), (8, 12)], 64) == [[0, 2], [1]]
    with pytest.raises(ValueError):
        EU.size_groups([(1, 1)], 0)


def test_similarity_is_the_mean_of_the_matrix_and_stars_are_stripped():
    ims, tok = _images(), _Tok()
    ev = EU.ImageDirEvaluator("cpu", clip_model=(_Vision(), _Text()), tokenizer=tok, max_batch=3)
    fs = torch.nn.functional.normalize(EU.encode_grouped(ims[:2], _Vision().forward_u8, "cpu"), dim=-1)
    fg = torch.nn.functional.normalize(EU.encode_grouped(ims[2:], _Vision().forward_u8, "cpu"), dim=-1)
    want_i = float(np.mean([[float(a @ b) for b in fg] for a in fs]))
    ft = torch.nn.functional.normalize(torch.tensor([1.0, 2.0, 0.0, 0.0]), dim=0)
    want_t = float(np.mean([float(ft @ b) for b in fg]))
    sim_i, sim_t = ev.evaluate(ims[2:], ims[:2], "a photo of a z * person*")
    assert abs(sim_i - want_i) < 1e-6 and abs(sim_t - want_t) < 1e-6
    assert tok.texts == [["a photo of a z  person"]]
    assert abs(ev.img_to_img_similarity(ims[:2], ims[:2]) - float((fs @ fs.T).mean())) < 1e-6
    assert ev.get_image_features(ims, norm=False).shape == (5, 4) and float(ev.get_image_features(ims).norm(dim=-1).max()) <= 1 + 1e-6
    dv = EU.ViTEvaluator("cpu", dino_model=_Vision(), max_batch=3)
    assert abs(dv.img_to_img_similarity(ims[:2], ims[2:]) - want_i) < 1e-6
    with pytest.raises(ValueError, match="not a file"):
        EU.CLIPEvaluator("cpu", clip_model="ViT-B/32")


def test_float_images_are_quantised_first():
    x = torch.tensor([-1.5, -1.0, -0.996, 0.0, 1.0 / 255, 3.0 / 255, 1.0, 2.0])          # 127.5 -> 128 and 128.5 -> 128, 129 exactly: ties to even
    img = x.view(1, 1, 1, 8).expand(1, 3, 1, 8)
    u8 = EU.float_images_to_u8(img)
    assert u8.shape == (1, 1, 8, 3) and u8.dtype == torch.uint8
    assert u8[0, 0, :, 0].tolist() == [0, 0, 1, 128, 128, 129, 255, 255]
    v = _Vision()
    EU.encode_grouped(img, v.forward_u8, "cpu")
    assert v.calls == [(1, 1, 8, 3)]
    assert [tuple(t.shape) for t in EU.images_to_u8_list(torch.zeros(2, 4, 5, 3, dtype=torch.uint8))] == [(4, 5, 3)] * 2
    with pytest.raises(ValueError):
        EU.images_to_u8_list(torch.zeros(2, 3, 4, 5, dtype=torch.uint8))


class _Extractor:
    """FaceIDExtractor's interface: an image whose first pixel is 0 shows no face; the ID is a unit vector chosen by that pixel."""

    def extract(self, images):
        ids, faceless = [], 0
        for im in images:
            k = int(load_rgb_u8(im)[0, 0, 0])                  # paths, PIL images and arrays, as FaceIDExtractor reads them
            if k == 0:
                faceless += 1
            else:
                ids.append(torch.nn.functional.one_hot(torch.tensor(k % 4), 4).float())
        return faceless, (torch.stack(ids) if ids else None)


def _face(k):
    return np.full((4, 4, 3), k, dtype=np.uint8)


def test_face_similarity_and_faceless_handling():
    ev = EU.FaceSimilarityEvaluator(_Extractor())
    assert ev.compare([_face(1), _face(2)], [_face(1), _face(0), _face(1)]) == (0.5, (0, 1))        # [[1, 1], [0, 0]] -> mean 0.5
    assert ev.compare([_face(1)], [_face(1)]) == (1.0, (0, 0))
    assert ev.compare([_face(0), _face(0)], [_face(1)]) == (0.0, (2, 0))
    assert ev.compare([_face(1)], [_face(0)]) == (0.0, (0, 1))
    assert ev.compare(torch.full((2, 4, 4, 3), 1, dtype=torch.uint8), [_face(1)]) == (1.0, (0, 0))


def test_compare_face_folders_reads_image_files(tmp_path):
    from PIL import Image
    for d, ks in (("a", (1, 2)), ("b", (1, 0))):
        (tmp_path / d).mkdir()
        for i, k in enumerate(ks):
            Image.fromarray(_face(k)).save(tmp_path / d / f"{i}.png")
    (tmp_path / "a" / "notes.txt").write_text("not an image")
    assert EU.compare_face_folders(str(tmp_path / "a"), str(tmp_path / "b"), _Extractor()) == (0.5, (0, 1))


# ---- af_vit_patch_rows: every refusal precedes the launch -----------------------------------------------------------------------------------
def test_patch_rows_argument_checks_without_a_gpu():
    L = _lib.lib()
    f3 = ctypes.c_float * 3
    sc, sh, P = f3(1, 1, 1), f3(0, 0, 0), 4096
    ok = dict(img=P, rows=2 * P, B=2, H=37, W=53, keep=1, S=16, C=16, p=8, filt=1, sc=sc, sh=sh, kpad=192)

    def call(**kw):
        a = dict(ok, **kw)
        return L.af_vit_patch_rows(a["img"], a["rows"], a["B"], a["H"], a["W"], a["keep"], a["S"], a["C"], a["p"], a["filt"], a["sc"], a["sh"], a["kpad"], None)

    bad = [dict(img=None), dict(rows=None), dict(sc=None), dict(sh=None), dict(C=12), dict(C=24, S=16), dict(kpad=184), dict(kpad=196), dict(filt=2),
           dict(filt=-1), dict(B=2 ** 20, H=32, W=32), dict(kpad=2 ** 28), dict(H=0), dict(p=0), dict(rows=2 * P + 8)]
    for kw in bad:
        assert call(**kw) == _lib.AF_E_BADARG, kw
        assert b"af_vit_patch_rows" in L.af_last_error(), kw
    assert call(keep=0, C=64, p=64, kpad=3 * 64 * 64) == _lib.AF_E_UNSUPPORTED and b"af_vit_patch_rows" in L.af_last_error()
    assert L.af_gelu_f16(None, P, 8, None) == _lib.AF_E_BADARG and L.af_gelu_f16(P, P, 0, None) == _lib.AF_E_BADARG
    assert b"af_gelu_f16" in L.af_last_error()
