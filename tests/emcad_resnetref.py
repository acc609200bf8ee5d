"""What the ResNet-encoder tests share: the fixture of tests/golden/make_golden_emcad_resnet.py and the model it describes.  Not a test module."""
import json
import os

import numpy as np
import torch

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = 9
CHANNELS = (2048, 1024, 512, 256)
BN3_GAMMA = 0.05          # as tests/golden/make_golden_emcad_resnet.py


def manifests():
    return json.load(open(os.path.join(G, "manifest_emcad_resnet.json")))


def reference_manifest():
    return manifests()["emcadnet_dual_k9_resnet50"]


def state_dict(seed=5):
    from oracle import weights as W
    return W.make_state_dict(reference_manifest(), seed=seed, bn3_gamma=BN3_GAMMA)


def build(encoder="resnet50", dual=True, pretrain=False):
    from lib.networks import EMCADNet
    return EMCADNet(num_classes=K, kernel_sizes=[1, 3, 5], expansion_factor=2, dw_parallel=True, add=True, lgag_ks=3, activation="relu6", encoder=encoder,
                    pretrain=pretrain, dual=dual)


_FIX = []


def fixture():
    """(z, x, label, bg_mask) of tests/golden/emcad_resnet50_128.npz, read once."""
    if not _FIX:
        z = np.load(os.path.join(G, "emcad_resnet50_128.npz"))
        z = {k: z[k] for k in z.files}
        label = torch.from_numpy(z["label"].astype(np.int64))
        bg = torch.stack([(label != k).float() for k in range(K)], 1)
        _FIX.append((z, torch.from_numpy(z["x"]), label, bg))
    return _FIX[0]
