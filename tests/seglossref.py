"""Float64 restatement of the single-supervision EMCAD loss (reference: multiclass_seg/EMCAD/trainer.py:113-119,141-153 with utils/utils.py DiceLoss(softmax=True))
in plain torch, and the helpers the single-supervision tests share.  Subsets and Dice come from oracle.emcad_oracle (powerset, dice_loss)."""
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import emcad_oracle as E
from oracle import weights as W

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ("mutation", "deep_supervision", "last")


def subsets(supervision, n=4):
    """The trainer's `ss` (trainer.py:113-119) as tuples of map indices."""
    if supervision == "mutation":
        return [tuple(s) for s in E.powerset(range(n)) if s]
    if supervision == "deep_supervision":
        return [(i,) for i in range(n)]
    if supervision == "last":
        return [(n - 1,)]                       # ss = [[-1]]
    raise ValueError(supervision)


def subset_mask(supervision):
    """15-bit mask of the kernels: bit s-1 selects subset s, bit i of s = map i is in the sum."""
    m = 0
    for s in subsets(supervision):
        m |= 1 << (sum(1 << i for i in s) - 1)
    return m


def seg_loss_ref(outs, label, supervision="mutation", weights=(0.3, 0.7)):
    """sum over the subsets of w_ce * CE(sum P_i) + w_dice * Dice(softmax(sum P_i)); outs: 4 (N,K,H,W) tensors (evaluated in their dtype: pass float64)."""
    K = outs[0].shape[1]
    loss = 0.0
    for s in subsets(supervision):
        iout = sum(outs[i] for i in s)
        loss = loss + weights[0] * F.cross_entropy(iout, label.long()) + weights[1] * E.dice_loss(iout, label, K)
    return loss


def single_manifest(num_classes=9):
    """state_dict keys -> shapes of EMCADNet(dual=False, encoder='pvt_v2_b2'): the dual manifest without the decoder's ConvBlock heads."""
    return OrderedDict((k, v) for k, v in W.manifest_emcadnet(num_classes).items() if not k.startswith("decoder.ConvBlock"))


def load_fixture():
    return np.load(os.path.join(G, "emcad_single_64.npz"))


def fixture_outs(z, pre=""):
    """The model outputs [p4, p3, p2, p1] of the fixture run `pre` ('' fp32, 'f64.' float64): the recorded out_head maps through the up-sampling of
    networks.py:134-137 (make_golden_emcad_single.py asserts that this reproduces the reference model's outputs bit for bit)."""
    return [F.interpolate(torch.from_numpy(z[f"{pre}head{i}"]), scale_factor=int(s), mode="bilinear") for i, s in enumerate(z["scales"])]
