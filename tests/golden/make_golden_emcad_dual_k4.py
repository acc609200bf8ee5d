"""Golden vectors for the dual EMCADNet at K = 4 classes with the PVTv2-B0 encoder (an ACDC-sized task) from the imported reference - build container only.
Runs in its own process, on make_golden_emcad.py's stubs and reference import, not on _ref_import.py: that helper imports
binary_seg, whose `lib` package has the name of multiclass_seg/EMCAD's own, and one process can hold only one of the two.

Data only: input, label, the eight low-resolution head maps of the decoder (fp32 and float64 runs) with the scale factors of networks.py:116-123, and the
reference's dual loss (trainer.py:109-140) in its three supervision modes, both precisions.  `out_i = F.interpolate(head_i, scale_factor=SCALES[i],
mode='bilinear')` is asserted here to reproduce the model's outputs bit for bit, and tests/duallossref.py:fixture_outs makes the same call.  The weights are
not stored: they follow from oracle.weights.make_state_dict(duallossref.manifest_b0(4), seed=5), whose key order and shapes are asserted against the model."""
import os, sys
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_emcad as G          # timm stubs + the reference's EMCADNet (imported from the reference tree)
import duallossref as D
from oracle import weights as W

K = 4
SCALES = (32, 16, 8, 4) * 2
LC = (0.5, 0.7, 0.3)                                    # trainer.py:127


def build(dtype):
    m = G.EMCADNet(num_classes=K, kernel_sizes=[1, 3, 5], expansion_factor=2, dw_parallel=True, add=True, lgag_ks=3, activation="relu6",
                   encoder="pvt_v2_b0", pretrain=False, dual=True)
    m.backbone.reset_drop_path(0.0)
    return m.to(dtype)


def main(size=64, n=2):
    for missing in ("medpy", "seaborn", "segmentation_mask_overlay", "SimpleITK", "thop", "ptflops"):
        G._stub(missing, metric=None, overlay_masks=None, profile=None, clever_format=None, get_model_complexity_info=None)
    cwd = os.getcwd(); os.chdir(G.REF)
    try:
        from utils.utils import powerset, DiceLoss
    finally:
        os.chdir(cwd)
    model = build(torch.float32)
    man = D.manifest_b0(K)
    assert [(k, list(v.shape)) for k, v in model.state_dict().items()] == [(k, list(v)) for k, v in man.items()], "manifest mismatch (EMCADNet dual, b0, K = 4)"
    sd0 = W.make_state_dict(man, seed=5)
    model.load_state_dict(sd0, strict=True)
    model.train()
    g = torch.Generator().manual_seed(77)
    x = torch.randn(n, 1, size, size, generator=g)
    label = torch.randint(0, K, (n, size, size), generator=g)
    label = F.interpolate(label[:, None, ::8, ::8].float(), size=(size, size), mode="nearest")[:, 0].long()      # blocky labels, as in emcad_single_64.npz
    bg_mask = torch.stack([(label != k).float() for k in range(K)], 1)
    out = {"x": G.npy(x), "label": G.npy(label).astype(np.uint8), "scales": np.asarray(SCALES)}
    out_idxs = list(range(4))
    SS = {"mutation": [s for s in powerset(out_idxs)], "deep_supervision": [[i] for i in out_idxs], "last": [[-1]]}      # trainer.py:113-119

    def run(m, xx, bgm, pre):
        heads = []
        hook = m.decoder.register_forward_hook(lambda mod, inp, o: heads.extend(t.detach().clone() for t in o))
        with torch.no_grad():
            P = m(xx, mode="train")
        hook.remove()
        assert len(P) == 8 and len(heads) == 8
        ce = nn.CrossEntropyLoss(); dl = DiceLoss(K); bce = nn.BCEWithLogitsLoss()
        P_fg, P_bg = P[:4], P[-4:]
        for mode, ss in SS.items():                           # trainer.py:123-140
            loss = 0.0
            for s in ss:
                iout, ibg = 0.0, 0.0
                if s == []:
                    continue
                for idx in range(len(s)):
                    iout = iout + P_fg[s[idx]]
                    ibg = ibg + P_bg[s[idx]]
                loss = loss + (LC[0] * ce(iout, label.long()) + LC[1] * dl(iout, label, softmax=True) + LC[2] * bce(ibg, bgm))
            out[pre + "loss." + mode] = G.npy(loss)
        for i, o in enumerate(P):
            assert torch.equal(F.interpolate(heads[i], scale_factor=SCALES[i], mode="bilinear"), o), i
            out[f"{pre}head{i}"] = G.npy(heads[i])
    run(model, x, bg_mask, "")
    m64 = build(torch.float32); m64.load_state_dict(sd0, strict=True); m64 = m64.double().train()
    run(m64, x.double(), bg_mask.double(), "f64.")
    path = os.path.join(HERE, "emcad_dual_k4_64.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "emcad_single_64.npz"))
    print("wrote emcad_dual_k4_64.npz", len(out), "arrays,", os.path.getsize(path), "bytes;",
          " ".join(f"{m} {float(out['loss.' + m]):.6f} (float64 {float(out['f64.loss.' + m]):.6f})" for m in SS))


if __name__ == "__main__":
    main()
