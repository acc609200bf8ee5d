"""Golden vectors for EMCADNet(dual, K=9) with the ResNet-50 encoder from the imported reference - build container only.  Runs in its own process:
multiclass_seg/EMCAD has its own `lib` package (same timm stubs as make_golden_emcad.py).

2 x 1 x 128^2: the deepest stage is 4 x 4 (make_golden_emcad_b0.py: at 64^2 train-mode BatchNorm over 8 values is ill-conditioned).  Weights from
oracle.weights.make_state_dict(manifest, seed=5, bn3_gamma=0.05) - none are stored.  bn3_gamma: the conditioned regime of make_golden_cond.py.  A plain random-init
BN-ReLU residual network of 16 blocks amplifies rounding noise: there the reference's own fp32 run sits 6e-4 .. 6e-3 from its float64 run on the train-mode maps, 7e-2 on
the eval-mode maps and 2.6 % on every backbone gradient, so a band of 3 on those distances would pass almost anything; with the last BatchNorm gamma of every
Bottleneck x 0.05 (the zero-init-residual regime of a trained checkpoint) they are 7e-6 .. 1.2e-4, 1.5e-5 and 0.17 %.  One train-mode step with the mutation loss in fp32 and in float64: the 8 float64 maps subsampled
(every 4th row and column) and rounded to fp32, `own.out{i}` = the reference's own fp32 distance to its float64 run on the full maps, the losses, 256-element gradient
probes with their norms and `own.gerr.<parameter>` (the fp32-to-float64 distance over the whole gradient tensor); then, with the BatchNorm running statistics that step
left, an eval-mode forward in both precisions (`eval.f64.out{i}`, `eval.own.out{i}`).  manifest_emcad_resnet.json: the state_dict layout of the model and the key / shape
lists of the reference's resnet101 and resnet152 backbones.

Prints every own.* figure (read them before committing a new fixture: an ill-conditioned probe shows as an own distance near the gradient's size); the reference's fp32
run is inside every gate of tests/test_gpu_emcad_resnet.py by construction - the gates are 3 x its own distances."""
import json, os, sys
import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_emcad as G          # timm stubs + the reference's EMCADNet (imported from the reference tree)
from oracle import weights as W

PROBES = ["conv.0.weight", "backbone.conv1.weight", "backbone.layer1.0.conv1.weight", "backbone.layer1.0.conv2.weight", "backbone.layer1.0.conv3.weight",
          "backbone.layer1.0.downsample.0.weight", "backbone.layer2.0.downsample.0.weight", "backbone.layer4.0.conv2.weight", "backbone.layer4.2.bn3.weight",
          "decoder.mscb4.0.pconv1.0.weight", "decoder.mscb1.0.pconv2.0.weight"]
NP = 256
SUB = 4
SUB_EVAL = 8          # the eval-mode maps: every 8th row and column
K = 9
BN3_GAMMA = 0.05          # oracle.weights.make_state_dict(bn3_gamma=): residual branches as small corrections, see the module docstring


def build(dtype):
    m = G.EMCADNet(num_classes=K, kernel_sizes=[1, 3, 5], expansion_factor=2, dw_parallel=True, add=True, lgag_ks=3, activation="relu6",
                   encoder="resnet50", pretrain=False, dual=True)
    return m.to(dtype)


def main(size=128, n=2):
    for missing in ("medpy", "seaborn", "segmentation_mask_overlay", "SimpleITK", "thop", "ptflops"):
        G._stub(missing, metric=None, overlay_masks=None, profile=None, clever_format=None, get_model_complexity_info=None)
    cwd = os.getcwd(); os.chdir(G.REF)
    try:
        from utils.utils import powerset, DiceLoss
        from lib.resnet import resnet101, resnet152
    finally:
        os.chdir(cwd)
    model = build(torch.float32)
    man = {k: list(v.shape) for k, v in model.state_dict().items()}
    layout = lambda m: [[k, list(v.shape)] for k, v in m.state_dict().items()]
    json.dump({"emcadnet_dual_k9_resnet50": man, "n_params": sum(p.numel() for p in model.parameters()),
               "resnet101": layout(resnet101()), "resnet152": layout(resnet152())}, open(os.path.join(HERE, "manifest_emcad_resnet.json"), "w"))
    sd0 = W.make_state_dict(man, seed=5, bn3_gamma=BN3_GAMMA)
    model.load_state_dict(sd0, strict=True)
    model.train()
    g = torch.Generator().manual_seed(77)
    x = torch.randn(n, 1, size, size, generator=g)
    label = torch.randint(0, K, (n, size, size), generator=g)
    label = torch.nn.functional.interpolate(label[:, None, ::8, ::8].float(), size=(size, size), mode="nearest")[:, 0].long()
    bg_mask = torch.stack([(label != k).float() for k in range(K)], 1)
    out = {"x": G.npy(x), "label": G.npy(label).astype(np.uint8), "sub": np.int64(SUB), "sub_eval": np.int64(SUB_EVAL)}

    def run(m, xx, bgm):
        P = m(xx, mode="train")
        ce = nn.CrossEntropyLoss(); dl = DiceLoss(K); bce = nn.BCEWithLogitsLoss()
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
        print(f"own.out{i} {float(out[f'own.out{i}']):.3e}  (|map| max {float(o64.detach().abs().max()):.3f})")
    out["loss"] = G.npy(loss).astype(np.float64); out["f64.loss"] = G.npy(l64)
    print(f"loss {float(loss):.8f} float64 {float(l64):.8f} own {abs(float(loss) - float(l64)):.3e}")
    for k in PROBES:
        g32, g64 = names[k].grad, n64[k].grad
        out["graw." + k] = G.npy(g32.reshape(-1)[:NP]); out["grawnorm." + k] = np.float64(g32.norm())
        out["f64.graw." + k] = G.npy(g64.reshape(-1)[:NP]); out["f64.grawnorm." + k] = G.npy(g64.norm())
        out["own.gerr." + k] = np.float64((g32.double() - g64).norm())
        head = float((g32.reshape(-1)[:NP].double() - g64.reshape(-1)[:NP]).norm())
        print(f"{k}: |g| {float(g64.norm()):.3e}  own norm err {abs(float(g32.norm()) - float(g64.norm())):.3e}  own.gerr {float(out['own.gerr.' + k]):.3e} "
              f"(rel {float(out['own.gerr.' + k]) / float(g64.norm()):.2e})  head |h| {float(g64.reshape(-1)[:NP].norm()):.3e} own head err {head:.3e}")
    # eval mode behind the step's running-statistics update (the weights are unchanged: no optimizer step)
    model.eval(); m64.eval()
    with torch.no_grad():
        E, E64 = model(x, mode="test"), m64(x.double(), mode="test")
    for i, (o, o64) in enumerate(zip(E, E64)):
        out[f"eval.f64.out{i}"] = G.npy(o64[:, :, ::SUB_EVAL, ::SUB_EVAL]).astype(np.float32)
        out[f"eval.own.out{i}"] = np.float64((o.double() - o64).abs().max())
        print(f"eval.own.out{i} {float(out[f'eval.own.out{i}']):.3e}")
    np.savez_compressed(os.path.join(HERE, "emcad_resnet50_128.npz"), **out)
    print("wrote emcad_resnet50_128.npz", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "emcad_resnet50_128.npz")), "bytes")


if __name__ == "__main__":
    main()
