"""PVT_CASCADE: EMCADNet's wrapper (lib/networks.py) around the CASCADE decoder (lib/cascade.py) - a PVTv2 encoder, CASCADE_Add_dual (dual=True: 8 K-class maps) or
CASCADE_Add / CASCADE_Cat + four out_head convs (dual=False: 4 maps; aggregation='additive' / 'concatenation', the reference networks' decoder_aggregation switch), bilinear
up-sampling by 32 / 16 / 8 / 4.  The reference has no dual-supervised concatenating decoder: every class that takes CASCADE_Cat puts plain heads behind it.

The reference pairs this decoder with MaxViT encoders (MIST_CAM, MERIT_*), which are not built here; it has no class of this name.  Parity for this class is therefore
against the composition of reference pieces (the PVTv2 encoder of multiclass_seg/EMCAD/lib/pvtv2.py, the decoder of MIST/lib/decoders.py, EMCADNet's input conv and
interpolation), not against a reference class.  Same contract as EMCADNet: _build_lowres, _build, hot_parameters, forward - Trainer(loss="mutation") and
pn2.infer.VolumePredictor take it unchanged."""
import os

import torch
import torch.nn as nn

from pn2 import F32
from pn2.graph import run_module
from lib import pvtv2
from lib.cascade import CASCADE_Add, CASCADE_Add_dual, CASCADE_Cat


class PVT_CASCADE(nn.Module):
    def __init__(self, num_classes=1, encoder='pvt_v2_b2', dual=True, pretrain=True, use_softmax=True, aggregation='additive'):
        super().__init__()
        if aggregation not in ('additive', 'concatenation'):
            raise ValueError(f"aggregation {aggregation!r}: 'additive' or 'concatenation'")
        if aggregation == 'concatenation' and dual:
            raise ValueError("aggregation='concatenation' needs dual=False: the concatenating decoder has no dual-supervised heads")
        self.dual = dual
        self.aggregation = aggregation
        self.conv = nn.Sequential(nn.Conv2d(1, 3, kernel_size=1), nn.BatchNorm2d(3), nn.ReLU(inplace=True))
        if encoder not in ('pvt_v2_b0', 'pvt_v2_b1', 'pvt_v2_b2', 'pvt_v2_b3', 'pvt_v2_b4', 'pvt_v2_b5'):
            raise NotImplementedError(f"encoder {encoder}: only the PVTv2 encoders are built")
        self.backbone = getattr(pvtv2, encoder)()
        path = f'./pretrained_pth/pvt/{encoder}.pth'
        channels = [256, 160, 64, 32] if encoder == 'pvt_v2_b0' else [512, 320, 128, 64]
        if pretrain is True and (os.path.exists(path) or os.environ.get('PN2_NO_PRETRAINED', '0') != '1'):
            save_model = torch.load(path)
            model_dict = self.backbone.state_dict()
            model_dict.update({k: v for k, v in save_model.items() if k in model_dict.keys()})
            self.backbone.load_state_dict(model_dict)
        if dual:
            self.decoder = CASCADE_Add_dual(channels=channels, num_class=num_classes, use_softmax=use_softmax)
        else:
            self.decoder = (CASCADE_Cat if aggregation == 'concatenation' else CASCADE_Add)(channels=channels)
        self.out_head4 = nn.Conv2d(channels[0], num_classes, 1)
        self.out_head3 = nn.Conv2d(channels[1], num_classes, 1)
        self.out_head2 = nn.Conv2d(channels[2], num_classes, 1)
        self.out_head1 = nn.Conv2d(channels[3], num_classes, 1)
        self.interpolation = 'bilinear'

    def hot_parameters(self, one_channel=True):
        """Parameters forward() touches: the out_head* convs only serve the single-supervision branch, the input conv only one-channel images."""
        return [p for n, p in self.named_parameters() if (not self.dual or not n.startswith('out_head')) and (one_channel or not n.startswith('conv.'))]

    def _build_lowres(self, eng, x):
        """-> (the 8 decoder head maps (dual) or [p4, p3, p2, p1] at 1/32, 1/16, 1/8, 1/4 of the input, their scale factors)"""
        if x.C == 1:
            x = eng.conv_bn_act(x, self.conv[0], self.conv[1], relu=True, bias=self.conv[0].bias)
        x1, x2, x3, x4 = self.backbone._build_features(eng, x)
        outs = self.decoder._build(eng, x4, [x3, x2, x1])
        if self.dual:
            return outs[:8], [32, 16, 8, 4] * 2          # (the ninth output, d1, has no head of its own)
        heads = [self.out_head4, self.out_head3, self.out_head2, self.out_head1]
        K = heads[0].out_channels
        return [eng.conv_bn_act(d, h, None, bias=h.bias, out_map=(K, (K + 7) // 8 * 8), y_dt=F32, y_C=K) for d, h in zip(outs, heads)], [32, 16, 8, 4]

    def _build(self, eng, x):
        lows, scales = self._build_lowres(eng, x)
        return [eng.bilinear(o, s) for o, s in zip(lows, scales)]

    def forward(self, x, mode='test'):
        return list(run_module(self._build, [x], self.hot_parameters(x.shape[1] == 1), self.training))
