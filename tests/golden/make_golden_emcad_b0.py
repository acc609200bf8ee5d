"""Golden vectors for EMCADNet(dual, K=9) with the PVTv2-B0 encoder (head_dim 32 in every stage) from the imported reference - build container
only.  Runs in its own process: multiclass_seg/EMCAD has its own `lib` package (same timm stubs as make_golden_emcad.py).

2 x 1 x 128^2: the deepest stage is 4 x 4 (at 64^2 it would be 2 x 2, where train-mode BatchNorm over 8 values is ill-conditioned).  The 8 maps
of the float64 run are stored subsampled (every 4th row and column) and rounded to fp32 (2^-24 relative, far below every gate), to keep the
file under 1 MB; `own.out{i}` is the reference's own fp32 distance to its float64 run, taken on the full maps."""
import json, os, sys
import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_emcad as G          # timm stubs + the reference's EMCADNet (imported from the reference tree)
from oracle import weights as W

PROBES = ["conv.0.weight", "backbone.patch_embed1.proj.weight", "backbone.block1.0.attn.q.weight", "backbone.block1.0.attn.kv.weight",
          "backbone.block1.0.attn.sr.weight", "backbone.block1.1.mlp.dwconv.dwconv.weight", "backbone.block2.1.attn.kv.weight",
          "backbone.block3.0.attn.proj.weight", "backbone.block4.1.attn.q.weight", "backbone.norm4.weight",
          "decoder.mscb4.0.pconv1.0.weight", "decoder.eucb1.pwc.0.weight", "decoder.lgag1.W_g.0.weight", "decoder.lgag1.W_x.0.bias",
          "decoder.lgag1.psi.0.weight", "decoder.cab1.fc1.weight", "decoder.cab1.fc2.weight", "decoder.mscb1.0.pconv1.0.weight",
          "decoder.mscb1.0.msdc.dwconvs.1.0.weight", "decoder.mscb1.0.pconv2.1.bias", "decoder.sab.conv.weight", "decoder.ConvBlock1_fg.conv.weight"]
NP = 256
SUB = 4


def build(dtype):
    m = G.EMCADNet(num_classes=9, kernel_sizes=[1, 3, 5], expansion_factor=2, dw_parallel=True, add=True, lgag_ks=3, activation="relu6",
                   encoder="pvt_v2_b0", pretrain=False, dual=True)
    m.backbone.reset_drop_path(0.0)
    return m.to(dtype)


def main(size=128, n=2):
    for missing in ("medpy", "seaborn", "segmentation_mask_overlay", "SimpleITK", "thop", "ptflops"):
        G._stub(missing, metric=None, overlay_masks=None, profile=None, clever_format=None, get_model_complexity_info=None)
    cwd = os.getcwd(); os.chdir(G.REF)
    try:
        from utils.utils import powerset, DiceLoss
    finally:
        os.chdir(cwd)
    model = build(torch.float32)
    man = {k: list(v.shape) for k, v in model.state_dict().items()}
    json.dump({"emcadnet_dual_k9_b0": man, "n_params": sum(p.numel() for p in model.parameters())}, open(os.path.join(HERE, "manifest_emcad_b0.json"), "w"))
    sd0 = W.make_state_dict(man, seed=5)
    model.load_state_dict(sd0, strict=True)
    model.train()
    g = torch.Generator().manual_seed(77)
    x = torch.randn(n, 1, size, size, generator=g)
    label = torch.randint(0, 9, (n, size, size), generator=g)
    label = torch.nn.functional.interpolate(label[:, None, ::8, ::8].float(), size=(size, size), mode="nearest")[:, 0].long()
    bg_mask = torch.stack([(label != k).float() for k in range(9)], 1)
    out = {"x": G.npy(x), "label": G.npy(label).astype(np.uint8), "sub": np.int64(SUB)}

    def run(m, xx, bgm):
        P = m(xx, mode="train")
        ce = nn.CrossEntropyLoss(); dl = DiceLoss(9); bce = nn.BCEWithLogitsLoss()
        loss = 0.0
        for s in powerset(list(range(4))):
            if s == []:
                continue
            iout = sum(P[i] for i in s); ibg = sum(P[4 + i] for i in s)
            loss = loss + 0.5 * ce(iout, label.long()) + 0.7 * dl(iout, label, softmax=True) + 0.3 * bce(ibg, bgm)
        loss.backward()
        return P, loss
    P, loss = run(model, x, bg_mask)
    names = dict(model.named_parameters())
    m64 = build(torch.float32); m64.load_state_dict(sd0, strict=True); m64 = m64.double().train()
    P64, l64 = run(m64, x.double(), bg_mask.double())
    n64 = dict(m64.named_parameters())
    for i, (o, o64) in enumerate(zip(P, P64)):
        out[f"f64.out{i}"] = G.npy(o64[:, :, ::SUB, ::SUB]).astype(np.float32)
        out[f"own.out{i}"] = np.float64((o.detach().double() - o64.detach()).abs().max())
    out["loss"] = G.npy(loss).astype(np.float64); out["f64.loss"] = G.npy(l64)
    for k in PROBES:
        out["graw." + k] = G.npy(names[k].grad.reshape(-1)[:NP]); out["grawnorm." + k] = np.float64(names[k].grad.norm())
        out["f64.graw." + k] = G.npy(n64[k].grad.reshape(-1)[:NP]); out["f64.grawnorm." + k] = G.npy(n64[k].grad.norm())
    np.savez_compressed(os.path.join(HERE, "emcad_b0_128.npz"), **out)
    print("wrote emcad_b0_128.npz", len(out), "arrays; loss", float(loss), "float64", float(l64))


if __name__ == "__main__":
    main()
