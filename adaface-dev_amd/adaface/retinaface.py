"""RetinaFace with a ResNet-50 backbone, the face detector the reference takes from ``retinaface.pre_trained_models`` (biubug6's
``Pytorch_Retinaface`` with ``cfg_re50``): photo -> boxes, confidences and five landmarks, for ``FaceIDExtractor(detect_faces=...)``
(``adaface/face_align.py``) and ``FaceCropper(detect_faces=...)`` (``ldm/modules/arcface_wrapper.py``).

Same module tree and parameter / buffer names as biubug6's ``RetinaFace`` (``body.*`` = torchvision ResNet-50 v1.5 without ``fc``, ``fpn.*``,
``ssh{1,2,3}.*``, ``ClassHead`` / ``BboxHead`` / ``LandmarkHead``), so ``Resnet50_Final.pth`` and ternaus' ``retinaface_resnet50_2020-07-20``
load with ``load_state_dict(strict=True)`` once an optional ``module.`` prefix is stripped (``load_retinaface_state_dict``).  The modules only
hold parameters; execution is NHWC fp16 through the C ABI, with the conventions of ``adaface/iresnet.py``:

* every BatchNorm follows its convolution and is folded into weights and bias;
* the 7x7 stride-2 stem is ``af_stem_im2col7x7`` (uint8 photo -> normalised rows, K = 147 in 160 columns) + one GEMM, then
  ``af_relu_maxpool3x3s2``; the image is padded at the bottom / right to multiples of 32 with zeros in normalised space, so every FPN level
  is exactly twice the next;
* 1x1 convolutions are ``ops.gemm`` on ``[B * H * W, C]`` rows, 3x3 convolutions ``ops.conv3x3`` (stride 2 on ``conv2`` of the first block
  of layers 2-4: ResNet v1.5); a stride-2 1x1 shortcut reads ``af_subsample2x``'s even pixels; the shortcut is added through ``residual=`` of
  the ``conv3`` GEMM;
* ReLU (LeakyReLU 0.1 for ``out_channel <= 64``) is ``ops.affine_prelu`` with a scalar slope -- the GEMM family has no ReLU epilogue;
* FPN top-down: ``af_upsample2x_add``;
* SSH: the two convolutions that read the block input (``conv3X3``, ``conv5X5_1``) are one convolution with N-concatenated weights, likewise
  ``conv5X5_2`` / ``conv7X7_2``; the block's final ReLU over the concatenation is applied to the pieces (ReLU is idempotent, so the piece
  that already had one is unchanged);
* the three heads of a level are ONE GEMM with N = 32.  Column layout, per anchor a in {0, 1}: 16 columns
  ``a * 16 + [box 0..3 | cls 0..1 | ldm 0..9]`` (rows ``a*4+k`` of ``BboxHead``, ``a*2+k`` of ``ClassHead``, ``a*10+k`` of ``LandmarkHead``),
  which is what ``af_retina_decode`` reads.

Frozen, eval-only, no backward (``inference_only``).  ``RetinaFaceDetector`` adds anchor decode, score filter and NMS on the device
(``af_retina_decode``, ``af_retina_nms``: a fixed-size table comes off the device in one copy) and the two callable contracts."""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..evaluation.arcface_resnet import _bn_affine, _fold_conv
from ..ops import F16

STRIDES = ops.RETINA_STEPS
PAD_TO = 32


def _conv_bn(inp, oup, k, stride=1, leaky=None):
    mods = [nn.Conv2d(inp, oup, k, stride, k // 2, bias=False), nn.BatchNorm2d(oup)]
    if leaky is not None:
        mods.append(nn.LeakyReLU(negative_slope=leaky, inplace=True))
    return nn.Sequential(*mods)


def _fold_1x1(conv, bn, dev):
    """1x1 convolution (+ the BatchNorm behind it) as a GEMM pack."""
    w = conv.weight.detach().float().flatten(1)
    b = None if conv.bias is None else conv.bias.detach().float()
    if bn is not None:
        s, t = _bn_affine(bn)
        w, b = w * s[:, None], t if b is None else b * s + t
    return ops.pack_matrix(w, b, dev)


def _fold_3x3_cat(pairs, dev):
    """Several (3x3 conv, BatchNorm) that read the same input as one convolution: output channels concatenated."""
    ws, bs = [], []
    for conv, bn in pairs:
        s, t = _bn_affine(bn)
        ws.append(conv.weight.detach().float() * s[:, None, None, None])
        bs.append(t)
    return ops.pack_conv3x3(torch.cat(ws), torch.cat(bs), dev)


def _rows(x):
    return x.reshape(-1, x.shape[-1])


class Bottleneck(nn.Module):
    """torchvision's Bottleneck (v1.5: the stride is on conv2)."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def pack(self, dev):
        return dict(conv1=_fold_1x1(self.conv1, self.bn1, dev), conv2=_fold_conv(self.conv2, self.bn2, dev),
                    conv3=_fold_1x1(self.conv3, self.bn3, dev),
                    down=None if self.downsample is None else _fold_1x1(self.downsample[0], self.downsample[1], dev))

    def hip(self, x, P, zero):
        B, H, W, _ = x.shape
        h = ops.affine_prelu(ops.gemm(_rows(x), P["conv1"]), slope=zero).reshape(B, H, W, -1)
        h = ops.affine_prelu(ops.conv3x3(h, P["conv2"], stride=self.stride), slope=zero)
        res = _rows(x)
        if P["down"] is not None:
            res = ops.gemm(_rows(ops.subsample2x(x)) if self.stride == 2 else res, P["down"])
        out = ops.affine_prelu(ops.gemm(_rows(h), P["conv3"], residual=res), slope=zero)
        return out.reshape(h.shape[0], h.shape[1], h.shape[2], -1)


class ResNetBody(nn.Module):
    """``IntermediateLayerGetter(resnet50, {layer2, layer3, layer4})``: conv1 .. layer4, no avgpool / fc."""

    def __init__(self, layers):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = self._make_layer(64, layers[0], 1)
        self.layer2 = self._make_layer(128, layers[1], 2)
        self.layer3 = self._make_layer(256, layers[2], 2)
        self.layer4 = self._make_layer(512, layers[3], 2)

    def _make_layer(self, planes, blocks, stride):
        downsample = None
        if stride != 1 or self.inplanes != planes * Bottleneck.expansion:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * Bottleneck.expansion, 1, stride, bias=False),
                                       nn.BatchNorm2d(planes * Bottleneck.expansion))
        layers = [Bottleneck(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * Bottleneck.expansion
        layers += [Bottleneck(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)


class FPN(nn.Module):
    def __init__(self, in_channels_list, out_channels):
        super().__init__()
        leaky = 0.1 if out_channels <= 64 else 0.0
        self.output1 = _conv_bn(in_channels_list[0], out_channels, 1, leaky=leaky)
        self.output2 = _conv_bn(in_channels_list[1], out_channels, 1, leaky=leaky)
        self.output3 = _conv_bn(in_channels_list[2], out_channels, 1, leaky=leaky)
        self.merge1 = _conv_bn(out_channels, out_channels, 3, leaky=leaky)
        self.merge2 = _conv_bn(out_channels, out_channels, 3, leaky=leaky)

    def pack(self, dev):
        P = {n: _fold_1x1(getattr(self, n)[0], getattr(self, n)[1], dev) for n in ("output1", "output2", "output3")}
        P.update({n: _fold_conv(getattr(self, n)[0], getattr(self, n)[1], dev) for n in ("merge1", "merge2")})
        return P

    def hip(self, feats, P, slope):
        lat = [ops.affine_prelu(ops.gemm(_rows(c), P[n]), slope=slope).reshape(c.shape[0], c.shape[1], c.shape[2], -1)
               for c, n in zip(feats, ("output1", "output2", "output3"))]
        o3 = lat[2]
        o2 = ops.affine_prelu(ops.conv3x3(ops.upsample2x_add(lat[1], o3), P["merge2"]), slope=slope)
        o1 = ops.affine_prelu(ops.conv3x3(ops.upsample2x_add(lat[0], o2), P["merge1"]), slope=slope)
        return [o1, o2, o3]


class SSH(nn.Module):
    def __init__(self, in_channel, out_channel):
        super().__init__()
        assert out_channel % 4 == 0
        leaky = 0.1 if out_channel <= 64 else 0.0
        self.conv3X3 = _conv_bn(in_channel, out_channel // 2, 3)
        self.conv5X5_1 = _conv_bn(in_channel, out_channel // 4, 3, leaky=leaky)
        self.conv5X5_2 = _conv_bn(out_channel // 4, out_channel // 4, 3)
        self.conv7X7_2 = _conv_bn(out_channel // 4, out_channel // 4, 3, leaky=leaky)
        self.conv7x7_3 = _conv_bn(out_channel // 4, out_channel // 4, 3)
        self.leaky, self.quarter = leaky, out_channel // 4

    def pack(self, dev):
        if self.leaky:                          # LeakyReLU is not idempotent under the final ReLU: every convolution on its own
            return {n: _fold_conv(getattr(self, n)[0], getattr(self, n)[1], dev)
                    for n in ("conv3X3", "conv5X5_1", "conv5X5_2", "conv7X7_2", "conv7x7_3")}
        return dict(first=_fold_3x3_cat([self.conv3X3[:2], self.conv5X5_1[:2]], dev), second=_fold_3x3_cat([self.conv5X5_2[:2], self.conv7X7_2[:2]], dev),
                    conv7x7_3=_fold_conv(self.conv7x7_3[0], self.conv7x7_3[1], dev))

    def hip(self, x, P, slope, zero):
        q = self.quarter
        if self.leaky:
            a = ops.conv3x3(x, P["conv3X3"])
            c = ops.affine_prelu(ops.conv3x3(x, P["conv5X5_1"]), slope=slope)
            b = ops.conv3x3(c, P["conv5X5_2"])
            d = ops.conv3x3(ops.affine_prelu(ops.conv3x3(c, P["conv7X7_2"]), slope=slope), P["conv7x7_3"])
            return ops.affine_prelu(torch.cat([a, b, d], dim=-1), slope=zero)
        # relu(cat[a, b, d]) = cat[relu(a), relu(b), relu(d)], and c = relu(conv5X5_1(x)), e = relu(conv7X7_2(c)) carry a ReLU anyway
        ac = ops.affine_prelu(ops.conv3x3(x, P["first"]), slope=zero)               # [.., 2q | q] = relu(conv3X3) | c
        be = ops.affine_prelu(ops.conv3x3(ac[..., 2 * q:].contiguous(), P["second"]), slope=zero)        # [.., q | q] = relu(conv5X5_2) | e
        d = ops.affine_prelu(ops.conv3x3(be[..., q:].contiguous(), P["conv7x7_3"]), slope=zero)
        return torch.cat([ac[..., :2 * q], be[..., :q], d], dim=-1)


class _Head(nn.Module):
    def __init__(self, inchannels, num_anchors, per_anchor):
        super().__init__()
        self.conv1x1 = nn.Conv2d(inchannels, num_anchors * per_anchor, kernel_size=1)


class ClassHead(_Head):
    def __init__(self, inchannels=512, num_anchors=3):
        super().__init__(inchannels, num_anchors, 2)


class BboxHead(_Head):
    def __init__(self, inchannels=512, num_anchors=3):
        super().__init__(inchannels, num_anchors, 4)


class LandmarkHead(_Head):
    def __init__(self, inchannels=512, num_anchors=3):
        super().__init__(inchannels, num_anchors, 10)


def _pack_heads(box, cls, ldm, dev):
    """One [32, C] matrix per level: per anchor a, rows a * 16 + [box 4 | cls 2 | ldm 10]."""
    ws, bs = [], []
    for a in range(2):
        for head, n in ((box, 4), (cls, 2), (ldm, 10)):
            ws.append(head.conv1x1.weight.detach().float().flatten(1)[a * n:(a + 1) * n])
            bs.append(head.conv1x1.bias.detach().float()[a * n:(a + 1) * n])
    return ops.pack_matrix(torch.cat(ws), torch.cat(bs), dev)


class RetinaFace(nn.Module):
    inference_only = True
    num_anchors = 2

    def __init__(self, layers=(3, 4, 6, 3), out_channel=256):
        super().__init__()
        self.body = ResNetBody(layers)
        in_list = [128 * Bottleneck.expansion, 256 * Bottleneck.expansion, 512 * Bottleneck.expansion]
        self.fpn = FPN(in_list, out_channel)
        self.ssh1, self.ssh2, self.ssh3 = SSH(out_channel, out_channel), SSH(out_channel, out_channel), SSH(out_channel, out_channel)
        self.ClassHead = nn.ModuleList([ClassHead(out_channel, self.num_anchors) for _ in range(3)])
        self.BboxHead = nn.ModuleList([BboxHead(out_channel, self.num_anchors) for _ in range(3)])
        self.LandmarkHead = nn.ModuleList([LandmarkHead(out_channel, self.num_anchors) for _ in range(3)])
        self.leaky = 0.1 if out_channel <= 64 else 0.0
        self._packs, self._packs_key = None, None
        self.eval()
        for p in self.parameters():
            p.requires_grad_(False)

    def blocks(self):
        for layer in (self.body.layer1, self.body.layer2, self.body.layer3, self.body.layer4):
            yield layer

    def _prepared(self):
        key = tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))
        if key != self._packs_key:
            w1 = self.body.conv1.weight
            dev = w1.device
            if not w1.is_cuda:
                raise RuntimeError("RetinaFace: parameters are on the CPU; this model only runs on an MI355X (HIP extension, no CPU "
                                   "fallback). Move it with .cuda() first.")
            s, t = _bn_affine(self.body.bn1)
            stem = torch.zeros((64, ops.STEM_COLS), device=dev)
            stem[:, :147] = (w1.detach().float() * s[:, None, None, None]).permute(0, 2, 3, 1).reshape(64, 147)      # (ky, kx, c)
            self._packs = dict(stem=ops.pack_matrix(stem, t, dev), layers=[[b.pack(dev) for b in layer] for layer in self.blocks()],
                               fpn=self.fpn.pack(dev), ssh=[m.pack(dev) for m in (self.ssh1, self.ssh2, self.ssh3)],
                               heads=[_pack_heads(self.BboxHead[k], self.ClassHead[k], self.LandmarkHead[k], dev) for k in range(3)],
                               zero=torch.zeros(1, device=dev), slope=torch.full((1,), self.leaky, device=dev))
            self._packs_key = key
        return self._packs

    def forward_heads(self, images_u8, scale, shift, bgr=False):
        """uint8 RGB photos [B, H, W, 3] on the device, normalised as ``v * scale[c] + shift[c]`` (``bgr``: channels swapped first) ->
        (three head tensors fp16 [B, Hk * Wk, 32] for strides 8, 16, 32, their (Hk, Wk)).  The image is padded to multiples of 32."""
        if self.training:
            raise NotImplementedError("RetinaFace runs frozen in eval mode (a face detector); training-mode BatchNorm is not implemented")
        P = self._prepared()                               # (raises for parameters on the CPU, before anything is launched)
        if images_u8.device != self.body.conv1.weight.device:
            raise RuntimeError(f"RetinaFace takes uint8 [B, H, W, 3] images on {self.body.conv1.weight.device}, got {tuple(images_u8.shape)} "
                               f"on {images_u8.device}")
        zero, slope = P["zero"], P["slope"]
        rows, (Ho, Wo) = ops.stem_im2col7x7(images_u8, scale, shift, bgr)
        B = images_u8.shape[0]
        h = ops.relu_maxpool3x3s2(ops.gemm(rows, P["stem"]).reshape(B, Ho, Wo, 64))
        feats = []
        for li, (layer, lp) in enumerate(zip(self.blocks(), P["layers"])):
            for blk, bp in zip(layer, lp):
                h = blk.hip(h, bp, zero)
            if li:
                feats.append(h)
        heads, sizes = [], []
        for f, ssh, sp, hp in zip(self.fpn.hip(feats, P["fpn"], slope), (self.ssh1, self.ssh2, self.ssh3), P["ssh"], P["heads"]):
            s = ssh.hip(f, sp, slope, zero)
            heads.append(ops.gemm(_rows(s), hp).reshape(B, -1, 32))
            sizes.append((f.shape[1], f.shape[2]))
        return heads, sizes

    def forward(self, images_u8, scale=(1.0, 1.0, 1.0), shift=(-104.0, -117.0, -123.0), bgr=True):
        """biubug6's outputs from uint8 photos: (bbox regressions [B, A, 4], class logits [B, A, 2] (NOT soft-maxed), landmark regressions
        [B, A, 10]), fp16, anchors in PriorBox order for the padded image."""
        heads, _ = self.forward_heads(images_u8, scale, shift, bgr)
        per_anchor = torch.cat([h.reshape(h.shape[0], -1, 16) for h in heads], dim=1)
        return per_anchor[..., :4], per_anchor[..., 4:6], per_anchor[..., 6:]


def load_retinaface_state_dict(model, state_dict):
    """``load_state_dict(strict=True)`` after stripping the ``module.`` prefix a DataParallel checkpoint (``Resnet50_Final.pth``) carries."""
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state_dict.items()}
    return model.load_state_dict(sd, strict=True)


PREPROCESS = {"biubug6": ((123.0, 117.0, 104.0), (1.0, 1.0, 1.0), True),                       # BGR, minus (104, 117, 123), no division
              "ternaus": (tuple(255.0 * m for m in (0.485, 0.456, 0.406)), tuple(255.0 * s for s in (0.229, 0.224, 0.225)), False)}


class RetinaFaceDetector:
    """``model``: a ``RetinaFace`` on the GPU.  ``preprocess``: ``"biubug6"`` (BGR order, minus (104, 117, 123)), ``"ternaus"`` (RGB,
    ImageNet mean / std on 0-255 values) or ``(mean_rgb, std_rgb, bgr)``.  An image whose longer side exceeds ``max_size`` is reduced on the
    host (PIL, bilinear) and its detections are scaled back; a smaller image is never enlarged.  At most ``max_det`` faces per image, best
    first.  The object is ``FaceIDExtractor``'s ``detect_faces``; ``detect_boxes`` is ``FaceCropper``'s."""

    def __init__(self, model, conf_threshold=0.7, nms_threshold=0.4, max_size=1024, preprocess="biubug6", max_det=64):
        if isinstance(preprocess, str):
            if preprocess not in PREPROCESS:
                raise ValueError(f"preprocess must be one of {sorted(PREPROCESS)} or (mean_rgb, std_rgb, bgr), got {preprocess!r}")
            preprocess = PREPROCESS[preprocess]
        mean, std, bgr = preprocess
        order = (2, 1, 0) if bgr else (0, 1, 2)                                  # network channel c reads RGB channel order[c]
        self.scale = tuple(1.0 / float(std[c]) for c in order)
        self.shift = tuple(-float(mean[c]) / float(std[c]) for c in order)
        self.bgr = bool(bgr)
        if not 1 <= int(max_det) <= ops.RETINA_CAPACITY:
            raise ValueError(f"max_det must be in [1, {ops.RETINA_CAPACITY}], got {max_det}")
        self.model, self.conf_threshold, self.nms_threshold = model, float(conf_threshold), float(nms_threshold)
        self.max_size, self.max_det = int(max_size), int(max_det)

    @property
    def device(self):
        return self.model.body.conv1.weight.device

    @torch.no_grad()
    def detect_batch(self, images_u8):
        """Device uint8 RGB [B, H, W, 3] -> host (table fp32 [B, max_det, 16], counts int32 [B, 2]): per image the kept detections, best
        first, as x1, y1, x2, y2, score, five (x, y) landmarks, anchor index, in pixels of the images as given; rows beyond ``kept`` are
        zero; counts = (kept, anchors that passed the confidence threshold)."""
        heads, sizes = self.model.forward_heads(images_u8, self.scale, self.shift, self.bgr)
        cand, count = ops.retina_decode(heads, sizes, self.conf_threshold)
        return ops.retina_nms(cand, count, self.nms_threshold, self.max_det)

    def _detect_one(self, image_rgb_u8):
        """-> rows [kept, 16] (float64) in pixels of the image it was given."""
        from .face_align import load_rgb_u8
        rgb = load_rgb_u8(image_rgb_u8.detach().cpu().numpy() if isinstance(image_rgb_u8, torch.Tensor) else image_rgb_u8)
        H, W, _ = rgb.shape
        bx = by = 1.0
        if max(H, W) > self.max_size:
            from PIL import Image
            r = self.max_size / max(H, W)
            size = (max(1, int(round(W * r))), max(1, int(round(H * r))))
            rgb = np.array(Image.fromarray(rgb).resize(size, Image.BILINEAR), dtype=np.uint8)
            bx, by = W / rgb.shape[1], H / rgb.shape[0]
        table, counts = self.detect_batch(torch.from_numpy(np.ascontiguousarray(rgb))[None].to(self.device))
        rows = table[0, :int(counts[0, 0])].double().numpy().copy()
        rows[:, [0, 2, 5, 7, 9, 11, 13]] *= bx
        rows[:, [1, 3, 6, 8, 10, 12, 14]] *= by
        return rows

    def __call__(self, image_rgb_u8):
        """``FaceIDExtractor``'s contract: uint8 [H, W, 3] RGB -> [(x, y, w, h, confidence, kps[5][2]), ...]."""
        return [(float(r[0]), float(r[1]), float(r[2] - r[0]), float(r[3] - r[1]), float(r[4]), r[5:15].reshape(5, 2).tolist())
                for r in self._detect_one(image_rgb_u8)]

    def detect_boxes(self, image_u8, T=20):
        """``FaceCropper``'s contract: -> [(x, y, w, h, confidence), ...] (it applies the size threshold ``T`` itself)."""
        return [f[:5] for f in self(image_u8)]
