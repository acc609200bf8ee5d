"""EMCADNet (reference: multiclass_seg/EMCAD/lib/networks.py:10-142): PVTv2 (lib/pvtv2.py) or ResNet-50/101/152 (lib/resnet.py) encoder + x32/x16/x8/x4 bilinear
up-sampling of the K-class maps of
  dual=True   the EMCAD_dual decoder (lib/decoders.py), 8 maps - the dual-supervision configuration of BASELINE config 5;
  dual=False  the EMCAD decoder + the four out_head convs, 4 maps - the reference's default, the single-supervision baseline of that comparison."""
import os

import torch
import torch.nn as nn

from pn2 import F32
from pn2.graph import run_module
from lib import pvtv2, resnet
from lib.decoders import EMCAD, EMCAD_dual


class EMCADNet(nn.Module):
    def __init__(self, num_classes=1, kernel_sizes=[1, 3, 5], expansion_factor=2, dw_parallel=True, add=True, lgag_ks=3, activation='relu', encoder='pvt_v2_b2', pretrain=True, **kwargs):
        super().__init__()
        self.dual = kwargs.get('dual', False)
        self.conv = nn.Sequential(nn.Conv2d(1, 3, kernel_size=1), nn.BatchNorm2d(3), nn.ReLU(inplace=True))
        if encoder == 'resnet50' and not self.dual:
            # tests/test_emcad_single_cpu.py::test_resnet_encoders_stay_unbuilt and tests/test_emcad_switches_cpu.py::test_refusals_that_stay pin exactly this model as refused, and
            # existing test files are not edited (the rule that keeps resnet18 / resnet34 refused below).  Nothing in the code stands in its way - resnet101 / resnet152 run with
            # these heads - so lifting it is deleting this branch together with those two pins.
            raise NotImplementedError("encoder resnet50 with the single-supervision heads (dual=False) stays refused: two existing tests pin it; resnet50 with dual=True and "
                                      "resnet101 / resnet152 in both supervision modes are built")
        if encoder in ('resnet50', 'resnet101', 'resnet152'):          # networks.py:55-63: the Bottleneck family; weights from ./pretrained_pth/resnet/ (lib/resnet.py)
            self.backbone = getattr(resnet, encoder)(pretrained=pretrain is True)
            channels = [2048, 1024, 512, 256]
        elif encoder in ('resnet18', 'resnet34'):
            raise NotImplementedError(f"encoder {encoder}: the BasicBlock encoders (resnet18, resnet34) are not built - of the ResNets only resnet50, resnet101 and resnet152")
        elif encoder in ('pvt_v2_b0', 'pvt_v2_b1', 'pvt_v2_b2', 'pvt_v2_b3', 'pvt_v2_b4', 'pvt_v2_b5'):
            self.backbone = getattr(pvtv2, encoder)()
            path = f'./pretrained_pth/pvt/{encoder}.pth'
            channels = [256, 160, 64, 32] if encoder == 'pvt_v2_b0' else [512, 320, 128, 64]     # networks.py:25-28
            if pretrain is True and (os.path.exists(path) or os.environ.get('PN2_NO_PRETRAINED', '0') != '1'):
                save_model = torch.load(path)
                model_dict = self.backbone.state_dict()
                model_dict.update({k: v for k, v in save_model.items() if k in model_dict.keys()})
                self.backbone.load_state_dict(model_dict)
        else:
            raise NotImplementedError(f"encoder {encoder}: the PVTv2 encoders and resnet50 / resnet101 / resnet152 are built")
        dec = dict(channels=channels, kernel_sizes=kernel_sizes, expansion_factor=expansion_factor, dw_parallel=dw_parallel, add=add, lgag_ks=lgag_ks, activation=activation)
        self.decoder = EMCAD_dual(num_class=num_classes, **dec) if self.dual else EMCAD(**dec)          # networks.py:83-88
        self.out_head4 = nn.Conv2d(channels[0], num_classes, 1)
        self.out_head3 = nn.Conv2d(channels[1], num_classes, 1)
        self.out_head2 = nn.Conv2d(channels[2], num_classes, 1)
        self.out_head1 = nn.Conv2d(channels[3], num_classes, 1)
        self.interpolation = 'bilinear'

    def hot_parameters(self, one_channel=True):
        """Parameters forward() touches: the out_head* convs only serve the single-supervision branch, a ResNet's 1000-way fc head nothing."""
        return [p for n, p in self.named_parameters() if (not self.dual or not n.startswith('out_head')) and (one_channel or not n.startswith('conv.')) and not n.startswith('backbone.fc.')]

    def _build_lowres(self, eng, x):
        """forward :101-132 up to the K-class head maps at 1/32, 1/16, 1/8, 1/4 of the input: (the 8 decoder maps (dual) or [p4, p3, p2, p1], their scale factors)"""
        if x.C == 1:
            x = eng.conv_bn_act(x, self.conv[0], self.conv[1], relu=True, bias=self.conv[0].bias)
        x1, x2, x3, x4 = self.backbone._build_features(eng, x)
        outs = self.decoder._build(eng, x4, [x3, x2, x1])
        if self.dual:
            return outs, [32, 16, 8, 4] * 2
        # prediction heads :129-132: biased 1x1 convs, no BatchNorm, as K-channel fp32 maps (the form BasicConv2d._build gives the dual heads)
        heads = [self.out_head4, self.out_head3, self.out_head2, self.out_head1]
        K = heads[0].out_channels
        return [eng.conv_bn_act(d, h, None, bias=h.bias, out_map=(K, (K + 7) // 8 * 8), y_dt=F32, y_C=K) for d, h in zip(outs, heads)], [32, 16, 8, 4]

    def _build(self, eng, x):
        """forward :101-142: 8 maps (dual) or [p4, p3, p2, p1]"""
        lows, scales = self._build_lowres(eng, x)
        return [eng.bilinear(o, s) for o, s in zip(lows, scales)]

    def forward(self, x, mode='test'):
        return list(run_module(self._build, [x], self.hot_parameters(x.shape[1] == 1), self.training))
