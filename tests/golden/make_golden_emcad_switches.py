"""Golden vectors for EMCADNet with the decoder switches away from their defaults (--concatenation, --no_dw_parallel, --lgag_ks 1, other --kernel_sizes and
--expansion_factor) from the imported reference - build container only.  Runs in its own process: multiclass_seg/EMCAD has its own `lib` package (same timm
stubs as make_golden_emcad.py).

Every configuration: pvt_v2_b0, K = 4, 2 x 1 x 128^2, DropPath off, weights from oracle.weights.make_state_dict(manifest, seed=5), train mode, the `mutation`
loss (dual: CE + Dice + BCE over the 15 subsets, trainer.py:123-140; single: CE + Dice, trainer.py:141-153), forward and backward in fp32 and in float64.
One emcad_sw_<name>.npz per configuration with what emcad_b0_128.npz stores (float64 maps subsampled by 4 as fp32, own.out{i} = the reference's own
fp32-to-float64 distance on the full maps, the losses, 256-element gradient probes with their norms) plus own.gerr.<parameter>, the reference's own
fp32-to-float64 distance over the whole gradient tensor (the bound of a norm's error: | |a| - |b| | <= |a - b|), and manifest_emcad_switches.json with the state_dict
keys and shapes of every configuration."""
import json, os, sys
import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_emcad as G          # timm stubs + the reference's EMCADNet (imported from the reference tree)
from oracle import weights as W

K = 4
NP = 256
SUB = 4
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
COMMON = ["conv.0.weight", "backbone.patch_embed1.proj.weight", "backbone.block1.0.attn.kv.weight", "backbone.norm4.weight",
          "decoder.mscb4.0.pconv1.0.weight", "decoder.mscb1.0.pconv1.0.weight", "decoder.mscb1.0.pconv2.0.weight", "decoder.mscb1.0.pconv2.1.bias",
          "decoder.mscb1.0.msdc.dwconvs.0.0.weight", "decoder.lgag1.W_g.0.weight", "decoder.lgag1.W_g.0.bias", "decoder.lgag1.W_x.0.weight",
          "decoder.lgag1.psi.0.weight", "decoder.eucb1.pwc.0.weight", "decoder.cab1.fc1.weight", "decoder.sab.conv.weight"]


def switches(name):
    return dict(DEFAULT, **CONFIGS[name][0])


def probes(name):
    last = len(switches(name)["kernel_sizes"]) - 1
    p = COMMON + [f"decoder.mscb1.0.msdc.dwconvs.{last}.0.weight", f"decoder.mscb4.0.msdc.dwconvs.{last}.1.weight"]
    p += ["decoder.ConvBlock1_fg.conv.weight"] if CONFIGS[name][1] else ["out_head4.weight", "out_head1.bias"]
    return list(dict.fromkeys(p))


def build(name, dtype):
    m = G.EMCADNet(num_classes=K, activation="relu6", encoder="pvt_v2_b0", pretrain=False, dual=CONFIGS[name][1], **switches(name))
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
    g = torch.Generator().manual_seed(77)
    x = torch.randn(n, 1, size, size, generator=g)
    label = torch.randint(0, K, (n, size, size), generator=g)
    label = torch.nn.functional.interpolate(label[:, None, ::8, ::8].float(), size=(size, size), mode="nearest")[:, 0].long()
    bg_mask = torch.stack([(label != k).float() for k in range(K)], 1)
    manifests = {}
    for name, (_, dual) in CONFIGS.items():
        model = build(name, torch.float32)
        man = {k: list(v.shape) for k, v in model.state_dict().items()}
        manifests[name] = man
        sd0 = W.make_state_dict(man, seed=5)
        model.load_state_dict(sd0, strict=True)
        model.train()
        out = {"x": G.npy(x), "label": G.npy(label).astype(np.uint8), "sub": np.int64(SUB)}

        def run(m, xx, bgm):
            P = m(xx, mode="train")
            ce = nn.CrossEntropyLoss(); dl = DiceLoss(K); bce = nn.BCEWithLogitsLoss()
            loss = 0.0
            for s in powerset(list(range(4))):
                if s == []:
                    continue
                iout = sum(P[i] for i in s)
                if dual:
                    loss = loss + 0.5 * ce(iout, label.long()) + 0.7 * dl(iout, label, softmax=True) + 0.3 * bce(sum(P[4 + i] for i in s), bgm)
                else:
                    loss = loss + 0.3 * ce(iout, label.long()) + 0.7 * dl(iout, label, softmax=True)
            loss.backward()
            return P, loss
        P, loss = run(model, x, bg_mask)
        assert len(P) == (8 if dual else 4)
        names = dict(model.named_parameters())
        m64 = build(name, torch.float32); m64.load_state_dict(sd0, strict=True); m64 = m64.double().train()
        P64, l64 = run(m64, x.double(), bg_mask.double())
        n64 = dict(m64.named_parameters())
        for i, (o, o64) in enumerate(zip(P, P64)):
            out[f"f64.out{i}"] = G.npy(o64[:, :, ::SUB, ::SUB]).astype(np.float32)
            out[f"own.out{i}"] = np.float64((o.detach().double() - o64.detach()).abs().max())
        out["loss"] = G.npy(loss).astype(np.float64); out["f64.loss"] = G.npy(l64)
        for k in probes(name):
            out["graw." + k] = G.npy(names[k].grad.reshape(-1)[:NP]); out["grawnorm." + k] = np.float64(names[k].grad.norm())
            out["f64.graw." + k] = G.npy(n64[k].grad.reshape(-1)[:NP]); out["f64.grawnorm." + k] = G.npy(n64[k].grad.norm())
            out["own.gerr." + k] = np.float64((names[k].grad.double() - n64[k].grad).norm())        # the reference's own fp32-to-float64 distance over the WHOLE gradient
        path = os.path.join(HERE, f"emcad_sw_{name}.npz")
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < 1000000, path
        print(f"wrote emcad_sw_{name}.npz", len(out), "arrays,", os.path.getsize(path), "bytes; loss", float(loss), "float64", float(l64))
    json.dump(manifests, open(os.path.join(HERE, "manifest_emcad_switches.json"), "w"))


if __name__ == "__main__":
    main()
