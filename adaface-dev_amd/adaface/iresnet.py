"""IResNet-50 / IResNet-100, the recogniser behind insightface's ArcFace models (``arcface_torch/backbones/iresnet.py``; the ``w600k_r50`` /
``glint360k_r100`` family), which turns an aligned 112x112 RGB crop into the 512-d face ID that Arc2Face and AdaFace start from.

Same module tree and parameter / buffer names as arcface_torch (``conv1``, ``bn1``, ``prelu``,
``layerN.M.{bn1,conv1,bn2,prelu,conv2,bn3,downsample.0,downsample.1}``, ``bn2``, ``fc``, ``features``), so a ``backbone.pth`` of that
family loads with ``load_state_dict(strict=True)``.  The modules only hold parameters; execution is NHWC fp16 through the C ABI, with the
conventions of ``evaluation/arcface_resnet.py`` (the ResNetFace-18 of the alignment loss):

* every convolution is the implicit-GEMM MFMA kernel with the eval-mode BatchNorm that FOLLOWS it folded into weights and bias
  (stem ``bn1``; block ``bn2`` / ``bn3``; the downsample BN), the 1x1 stride-2 shortcut as the centre tap of a 3x3 stride-2 filter, and the
  shortcut added in the second convolution's epilogue;
* a block's ``bn1`` precedes a zero-padded conv, so it cannot be folded (the shift would leak into the border): ``af_affine_prelu_ch``,
  which is also the PReLU with one slope per channel (``nn.PReLU(planes)``);
* ``bn2 -> dropout (eval: identity) -> flatten (NCHW order) -> fc -> features`` collapses into one GEMM on NHWC-ordered, pre-scaled
  weights.

Frozen and in eval mode; training-mode BatchNorm statistics / Dropout raise.  There is no backward (``inference_only``): this network reads
photos, nothing differentiates through it."""
import torch
import torch.nn as nn

from .. import ops
from ..evaluation.arcface_resnet import _bn_affine, _fold_conv, conv3x3
from ..ops import F16

WIDTHS = (64, 128, 256, 512)
CROP = 112                          # input side; four stride-2 layers leave 7 x 7 (fc is 512 * 7 * 7 wide)


def _f32(t, dev):
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


class IBasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(inplanes, eps=1e-05)
        self.conv1 = conv3x3(inplanes, planes)
        self.bn2 = nn.BatchNorm2d(planes, eps=1e-05)
        self.prelu = nn.PReLU(planes)
        self.conv2 = conv3x3(planes, planes, stride)
        self.bn3 = nn.BatchNorm2d(planes, eps=1e-05)
        self.downsample = downsample
        self.stride = stride

    def pack(self, dev):
        s1, t1 = _bn_affine(self.bn1)
        return dict(bn1=(_f32(s1, dev), _f32(t1, dev)), conv1=_fold_conv(self.conv1, self.bn2, dev), slope=_f32(self.prelu.weight, dev),
                    conv2=_fold_conv(self.conv2, self.bn3, dev),
                    down=None if self.downsample is None else _fold_conv(self.downsample[0], self.downsample[1], dev))

    def hip(self, x, P):
        out = ops.conv3x3(ops.affine_prelu_ch(x, P["bn1"][0], P["bn1"][1]), P["conv1"])
        out = ops.affine_prelu_ch(out, slope=P["slope"])
        res = x if P["down"] is None else ops.conv3x3(x, P["down"], stride=self.stride)
        return ops.conv3x3(out, P["conv2"], stride=self.stride, residual=res)


class IResNet(nn.Module):
    inference_only = True        # no input gradient: ArcFaceWrapper refuses it for a tensor that needs one
    fc_scale = 7 * 7

    def __init__(self, block=IBasicBlock, layers=(3, 13, 30, 3), dropout=0, num_features=512):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, self.inplanes, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(self.inplanes, eps=1e-05)
        self.prelu = nn.PReLU(self.inplanes)
        self.layer1 = self._make_layer(block, WIDTHS[0], layers[0], stride=2)
        self.layer2 = self._make_layer(block, WIDTHS[1], layers[1], stride=2)
        self.layer3 = self._make_layer(block, WIDTHS[2], layers[2], stride=2)
        self.layer4 = self._make_layer(block, WIDTHS[3], layers[3], stride=2)
        self.bn2 = nn.BatchNorm2d(512 * block.expansion, eps=1e-05)
        self.dropout = nn.Dropout(p=dropout, inplace=True)
        self.fc = nn.Linear(512 * block.expansion * self.fc_scale, num_features)
        self.features = nn.BatchNorm1d(num_features, eps=1e-05)
        nn.init.constant_(self.features.weight, 1.0)
        self.features.weight.requires_grad = False
        for m in self.modules():                                              # arcface_torch's initialisation
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, 0, 0.1)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        self.num_features = num_features
        self._packs, self._packs_key = None, None

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                                       nn.BatchNorm2d(planes * block.expansion, eps=1e-05))
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes))
        return nn.Sequential(*layers)

    def blocks(self):
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            yield from layer

    def _prepared(self):
        key = tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))
        if key != self._packs_key:
            dev = self.conv1.weight.device
            if not self.conv1.weight.is_cuda:
                raise RuntimeError("IResNet: parameters are on the CPU; this model only runs on an MI355X (HIP extension, no CPU "
                                   "fallback). Move it with .cuda() first.")
            nf, c, hw = self.num_features, self.bn2.num_features, self.fc_scale
            side = int(round(hw ** 0.5))
            s2, t2 = _bn_affine(self.bn2)
            sf, tf = _bn_affine(self.features)
            w = self.fc.weight.detach().float().reshape(nf, c, side, side)            # columns in NCHW flatten order
            b = self.fc.bias.detach().float() + (w * t2[None, :, None, None]).sum(dim=(1, 2, 3))
            w = (w * s2[None, :, None, None]).permute(0, 2, 3, 1).reshape(nf, hw * c)    # -> NHWC flatten order
            self._packs = dict(conv1=_fold_conv(self.conv1, self.bn1, dev, cin_pad=8), slope=_f32(self.prelu.weight, dev),
                               blocks=[b_.pack(dev) for b_ in self.blocks()], fc=ops.pack_matrix(w * sf[:, None], b * sf + tf, dev))
            self._packs_key = key
        return self._packs

    def _check(self, x, shape):
        if self.training:
            raise NotImplementedError("IResNet runs frozen in eval mode (a face-ID extractor); training-mode BatchNorm / Dropout are not "
                                      "implemented")
        P = self._prepared()                               # (raises for parameters on the CPU, before anything is launched)
        if tuple(x.shape[1:]) != shape or x.device != self.conv1.weight.device:
            raise RuntimeError(f"IResNet takes [B, {', '.join(map(str, shape))}] crops on {self.conv1.weight.device} (fc is 512*7*7 wide), got "
                               f"{tuple(x.shape)} on {x.device}")
        return P

    def forward_nhwc(self, x):
        """Aligned crops as ``ops.face_align_crop`` writes them, fp16 [B, 112, 112, 8] (RGB in channels 0-2, zeros in 3-7) -> fp16 [B, 512]."""
        P = self._check(x, (CROP, CROP, 8))
        h = ops.affine_prelu_ch(ops.conv3x3(x, P["conv1"]), slope=P["slope"])
        for blk, bp in zip(self.blocks(), P["blocks"]):
            h = blk.hip(h, bp)
        return ops.gemm(h.reshape(x.shape[0], -1), P["fc"])                          # bn2 . flatten . fc . features

    def forward(self, x):
        """[B, 3, 112, 112] crops scaled to [-1, 1] (arcface_torch's input) -> [B, 512] in x's dtype."""
        self._check(x, (3, CROP, CROP))
        y = self.forward_nhwc(ops.nchw_f32_to_nhwc_f16(x.detach().float().contiguous(), cpad=8))
        return y if x.dtype == F16 else y.to(x.dtype)


def iresnet50(**kwargs):
    return IResNet(IBasicBlock, (3, 4, 14, 3), **kwargs)


def iresnet100(**kwargs):
    return IResNet(IBasicBlock, (3, 13, 30, 3), **kwargs)
