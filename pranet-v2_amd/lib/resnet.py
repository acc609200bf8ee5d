"""ResNet-50 / 101 / 152 encoders of EMCADNet on the pn2 engine.

Same class / function names, constructor arguments, attribute names and state_dict keys as the reference's multiclass_seg/EMCAD/lib/resnet.py (Bottleneck :64-100,
ResNet :103-179, factories :214-248), so torchvision-style checkpoints and `model.backbone.layerN` access carry over.  nn.Conv2d / nn.BatchNorm2d leaves are
parameter containers; the arithmetic runs in the gfx950 kernels via `_build` (NHWC).

Built: the Bottleneck family with the plain 7x7 stem.  Not built: BasicBlock and its factories (resnet18 / resnet34 - EMCADNet refuses them) and the deep_base stem,
which no reference script sets.  Pretrained weights are read from disk only (./pretrained_pth/resnet/<name>.pth); nothing here fetches anything.
"""
import math
import os

import torch
import torch.nn as nn

from pn2.graph import run_module

__all__ = ['ResNet', 'resnet50', 'resnet101', 'resnet152']


def POOL_FUSE():
    from pn2 import core
    return core.POOL_FUSE


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * Bottleneck.expansion, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * Bottleneck.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def _build(self, eng, x):
        """Reference Bottleneck.forward (resnet.py:80-100) expressed in engine ops."""
        # x_last as in Bottle2neck._build: conv1 is the first consumer of the block input (the skip - identity, downsample conv or strided gather - comes later in forward
        # order, so its gradient arrives earlier); conv2 and conv3 sit on single-consumer chains
        out = eng.conv_bn_act(x, self.conv1, self.bn1, relu=True, x_last=True)
        out = eng.conv_bn_act(out, self.conv2, self.bn2, relu=True, x_last=True)
        if self.downsample is not None:
            dconv, dbn = self.downsample[0], self.downsample[1]
            # (defer_out: conv3 below is the only reader of the downsample BatchNorm's output - in a training pass it is never written, conv3's output pass normalises both)
            if dconv.stride[0] == 1:          # layer1: 64 -> 256 at the block's own extent
                res = eng.conv_bn_act(x, dconv, dbn, defer_out=True)
            else:                             # layer2..4: the 1x1 conv reads one pixel in four - gathered first, then the stride-1 pointwise path
                res = eng.strided_pointwise(x, dconv, dbn, defer_out=True)
        else:
            res = x
        return eng.conv_bn_act(out, self.conv3, self.bn3, relu=True, residual=res, x_last=True)

    def forward(self, x):
        return run_module(lambda e, a: [self._build(e, a)], [x], list(self.parameters()), self.training)[0]


class ResNet(nn.Module):
    def __init__(self, block, layers, num_classes=1000, deep_base=False, stem_width=32):
        if deep_base:
            raise NotImplementedError("ResNet(deep_base=True): the three-conv stem is not built (no reference script sets it)")
        self.inplanes = 64
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(self.inplanes)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)
        self.avgpool = nn.AvgPool2d(7, stride=1)
        self.fc = nn.Linear(512 * block.expansion, num_classes)          # (kept for the checkpoints' sake: the features never reach it, resnet.py:175-177)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / n))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                nn.Conv2d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                nn.BatchNorm2d(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes))
        return nn.Sequential(*layers)

    def _build_features(self, eng, x):
        """stem + maxpool + layer1..4 -> [layer1, layer2, layer3, layer4] (resnet.py:158-179)."""
        if eng.training and POOL_FUSE():
            # bn1 -> relu -> maxpool as one op, as in the Res2Net stem: the half-resolution BatchNorm output is consumed by the pool alone and never written.  Behind
            # EMCADNet's 1 -> 3 input conv the data gradient of this 7x7 / stride-2 conv takes the per-pixel few-channel path (ConvOps._conv_bwd: 49 x 64 float4 of LDS)
            x = eng.conv_bn_act(x, self.conv1, self.bn1, relu=True, pool=True)
        else:
            x = eng.conv_bn_act(x, self.conv1, self.bn1, relu=True)
            x = eng.maxpool3x3s2(x)
        feats = []
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                x = blk._build(eng, x)
            feats.append(x)
        return feats

    def hot_parameters(self):
        """Parameters the features touch: everything but the 1000-way head."""
        return [p for n, p in self.named_parameters() if not n.startswith('fc.')]

    def forward(self, x):
        return list(run_module(lambda e, a: self._build_features(e, a), [x], self.hot_parameters(), self.training))


def _load_pretrained(model, name):
    """The reference fetches these checkpoints (resnet.py:221-247); here they are read from a fixed relative path, under the rule of the PVTv2 branch of lib/networks.py:
    a missing file is an error unless PN2_NO_PRETRAINED=1 (benchmarks / tests use random init)."""
    path = f'./pretrained_pth/resnet/{name}.pth'
    if os.path.exists(path) or os.environ.get('PN2_NO_PRETRAINED', '0') != '1':
        model.load_state_dict(torch.load(path))
    return model


def resnet50(pretrained=False, **kwargs):
    model = ResNet(Bottleneck, [3, 4, 6, 3], **kwargs)
    return _load_pretrained(model, 'resnet50') if pretrained else model


def resnet101(pretrained=False, **kwargs):
    model = ResNet(Bottleneck, [3, 4, 23, 3], **kwargs)
    return _load_pretrained(model, 'resnet101') if pretrained else model


def resnet152(pretrained=False, **kwargs):
    model = ResNet(Bottleneck, [3, 8, 36, 3], **kwargs)
    return _load_pretrained(model, 'resnet152') if pretrained else model
