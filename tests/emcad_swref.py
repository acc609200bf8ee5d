"""The decoder-switch configurations of tests/golden/make_golden_emcad_switches.py (same names, same switches) and their fixtures, shared by
test_emcad_switches_cpu.py and test_gpu_emcad_switches.py."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = 4
DEFAULT = dict(kernel_sizes=[1, 3, 5], expansion_factor=2, dw_parallel=True, add=True, lgag_ks=3)
_ALL = dict(kernel_sizes=[1, 3], add=False, dw_parallel=False, lgag_ks=1, expansion_factor=6)
CONFIGS = {                                             # name -> (switches changed from the default, dual)
    "cat": (dict(add=False), True),
    "seq": (dict(dw_parallel=False), True),
    "lgag1": (dict(lgag_ks=1), True),
    "k333": (dict(kernel_sizes=[3, 3, 3]), True),
    "k1355": (dict(kernel_sizes=[1, 3, 5, 5]), True),
    "all": (_ALL, True),
    "all_single": (_ALL, False),
}
NAMES = list(CONFIGS)
_CACHE = {}


def switches(name):
    return dict(DEFAULT, **CONFIGS[name][0])


def manifest(name):
    if "manifest" not in _CACHE:
        _CACHE["manifest"] = json.load(open(os.path.join(GOLDEN, "manifest_emcad_switches.json")))
    return _CACHE["manifest"][name]


def build(name):
    """EMCADNet of the configuration with the fixture's weights (oracle.weights.make_state_dict(manifest, seed=5)), DropPath off, on the CPU."""
    from lib.networks import EMCADNet
    from oracle import weights as W
    m = EMCADNet(num_classes=K, activation="relu6", encoder="pvt_v2_b0", pretrain=False, dual=CONFIGS[name][1], **switches(name))
    m.load_state_dict(W.make_state_dict(manifest(name), seed=5), strict=True)
    m.backbone.reset_drop_path(0.0)
    return m


def fixture(name):
    """-> (npz, x, label, bg_mask); loaded once per configuration and never modified"""
    if name not in _CACHE:
        z = np.load(os.path.join(GOLDEN, f"emcad_sw_{name}.npz"))
        label = torch.from_numpy(z["label"].astype(np.int64))
        _CACHE[name] = (z, torch.from_numpy(z["x"]), label, torch.stack([(label != k).float() for k in range(K)], 1))
    return _CACHE[name]
