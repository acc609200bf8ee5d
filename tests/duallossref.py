"""Float64 restatement of the dual-supervision EMCAD loss for any class count, any (lc1, lc2, lc3) and every supervision mode (reference:
multiclass_seg/EMCAD/trainer.py:109-140 with utils/utils.py DiceLoss(softmax=True)) in plain torch, and the helpers the dual-loss tests share.  Subsets and Dice
come from oracle.emcad_oracle (powerset, dice_loss) through seglossref.subsets.  Not a test module."""
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import seglossref as R
from oracle import emcad_oracle as E

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = R.MODES
LC = (0.5, 0.7, 0.3)                                         # trainer.py:127
PVT_B0 = dict(embed_dims=(32, 64, 160, 256), num_heads=(1, 2, 5, 8), mlp_ratios=(8, 8, 4, 4), depths=(2, 2, 2, 2), sr_ratios=(8, 4, 2, 1))
CHANNELS = (256, 160, 64, 32)


def dual_loss_ref(outs, label, bg_mask, supervision="mutation", lc=LC):
    """trainer.py:123-140: sum over the subsets s of lc1 * CE(sum_{i in s} fg_i) + lc2 * Dice(softmax(sum fg_i)) + lc3 * BCEWithLogits(sum_{i in s} bg_i, bg_mask);
    outs: 8 (N,K,H,W) tensors, P_fg = outs[:4], P_bg = outs[-4:] (evaluated in their dtype: pass float64)."""
    if len(outs) != 8:
        raise ValueError(len(outs))
    P_fg, P_bg = outs[:4], outs[-4:]
    K = outs[0].shape[1]
    loss = 0.0
    for s in R.subsets(supervision):
        iout = sum(P_fg[i] for i in s); ibg = sum(P_bg[i] for i in s)
        loss = loss + lc[0] * F.cross_entropy(iout, label.long()) + lc[1] * E.dice_loss(iout, label, K) \
            + lc[2] * F.binary_cross_entropy_with_logits(ibg, bg_mask.to(ibg.dtype))
    return loss


def bg_mask_of(label, K):
    """The reference's background mask: the inverted one-hot of the label, (N,K,H,W)."""
    return torch.stack([(label != k).float() for k in range(K)], 1)


def manifest_b0(num_classes):
    """EMCADNet(dual=True, encoder='pvt_v2_b0') key -> shape in state_dict() order, from the oracle's generic manifest pieces (tests/emcad_b0ref.py at K = 9)."""
    from oracle import weights as W
    m = OrderedDict()
    W._conv(m, "conv.0", 3, 1, 1, 1, bias=True); W._bn(m, "conv.1", 3)
    W._pvt_v2(m, "backbone.", cfg=PVT_B0)
    W._emcad_decoder(m, "decoder.", channels=CHANNELS, num_class=num_classes)
    for i, cch in zip((4, 3, 2, 1), CHANNELS):
        W._conv(m, f"out_head{i}", num_classes, cch, 1, 1, bias=True)
    return m


def load_fixture():
    return np.load(os.path.join(G, "emcad_dual_k4_64.npz"))


def fixture_outs(z, pre=""):
    """The 8 model outputs of the fixture run `pre` ('' fp32, 'f64.' float64): the recorded low-resolution head maps through the up-sampling of
    networks.py (make_golden_emcad_dual_k4.py asserts that this reproduces the reference model's outputs bit for bit)."""
    return [F.interpolate(torch.from_numpy(z[f"{pre}head{i}"]), scale_factor=int(s), mode="bilinear") for i, s in enumerate(z["scales"])]
