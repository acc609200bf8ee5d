"""The EMCADNet(dual, K=9, pvt_v2_b0) restatement the b0 tests share: the generic oracle pieces composed with the b0 configuration
(pvtv2.py:378-384, networks.py:25-28).  Not a test module."""
import json
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PVT_B0 = dict(embed_dims=(32, 64, 160, 256), num_heads=(1, 2, 5, 8), mlp_ratios=(8, 8, 4, 4), depths=(2, 2, 2, 2), sr_ratios=(8, 4, 2, 1))
CHANNELS = (256, 160, 64, 32)


def manifest():
    """EMCADNet(dual, K=9, pvt_v2_b0) key -> shape in state_dict() order, built from the oracle's generic manifest pieces."""
    from oracle import weights as W
    m = OrderedDict()
    W._conv(m, "conv.0", 3, 1, 1, 1, bias=True); W._bn(m, "conv.1", 3)
    W._pvt_v2(m, "backbone.", cfg=PVT_B0)
    W._emcad_decoder(m, "decoder.", channels=CHANNELS, num_class=9)
    for i, cch in zip((4, 3, 2, 1), CHANNELS):
        W._conv(m, f"out_head{i}", 9, cch, 1, 1, bias=True)
    return m


def reference_manifest():
    return json.load(open(os.path.join(G, "manifest_emcad_b0.json")))["emcadnet_dual_k9_b0"]


def state_dict(seed=5):
    from oracle import weights as W
    return W.make_state_dict(reference_manifest(), seed=seed)


def forward(P, x, training=True):
    """oracle.emcad_oracle.emcadnet_forward with the b0 encoder configuration."""
    from oracle.pranet_oracle import Ctx, bn, pvt_features
    from oracle import emcad_oracle as E
    ctx = Ctx(training)
    x = F.relu(bn(P, "conv.1", F.conv2d(x, P["conv.0.weight"], P["conv.0.bias"]), ctx))
    x1, x2, x3, x4 = pvt_features(P, "backbone.", x, PVT_B0)
    outs = E.emcad_dual(P, "decoder.", x4, [x3, x2, x1], ctx)
    return [F.interpolate(o, scale_factor=s, mode="bilinear") for o, s in zip(outs, [32, 16, 8, 4] * 2)]


def fixture():
    """(z, x, label, bg_mask) of tests/golden/emcad_b0_128.npz (make_golden_emcad_b0.py)."""
    z = np.load(os.path.join(G, "emcad_b0_128.npz"))
    label = torch.from_numpy(z["label"].astype(np.int64))
    bg = torch.stack([(label != k).float() for k in range(9)], 1)
    return z, torch.from_numpy(z["x"]), label, bg
