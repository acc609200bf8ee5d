"""Golden vectors for the single-supervision EMCADNet (dual left at its default False, K=9) from the imported reference — build container only.
Runs in its own process: multiclass_seg/EMCAD has its own `lib` package, which would collide with binary_seg's.

The four full-resolution maps are recorded as what they are made of: the low-resolution out_head outputs `head0..3` (captured with forward hooks) and the
scale factors of networks.py:134-137.  `out_i = F.interpolate(head_i, scale_factor=SCALES[i], mode='bilinear')` is asserted here to reproduce the model's
output bit for bit, in fp32 and in float64, and tests/seglossref.py:fixture_outs makes the same call; eight 2 x 9 x 64 x 64 maps would not fit a committed file."""
import json, os, sys, types
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
REF = "/root/reference/multiclass_seg/EMCAD"


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


class DropPath(nn.Module):
    def __init__(self, drop_prob=0.0):
        super().__init__(); self.drop_prob = drop_prob
    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        raise RuntimeError("golden vectors are generated with DropPath off")


def named_apply(fn, module, name="", depth_first=True, include_root=False):
    if not depth_first and include_root:
        fn(module=module, name=name)
    for cn, cm in module.named_children():
        named_apply(fn=fn, module=cm, name=".".join((name, cn)) if name else cn, depth_first=depth_first, include_root=True)
    if depth_first and include_root:
        fn(module=module, name=name)
    return module


tn = lambda t, std=1.0, **k: nn.init.trunc_normal_(t, std=std, a=-2, b=2)
_stub("timm"); _stub("timm.models")
_stub("timm.models.layers", DropPath=DropPath, to_2tuple=lambda x: tuple(x) if isinstance(x, (tuple, list)) else (x, x), trunc_normal_=tn, trunc_normal_tf_=tn)
_stub("timm.models.helpers", named_apply=named_apply)
_stub("timm.models.registry", register_model=lambda f: f)
_stub("timm.models.vision_transformer", _cfg=lambda **k: {})
sys.path.insert(0, REF)
cwd = os.getcwd(); os.chdir(REF)
try:
    from lib.networks import EMCADNet
finally:
    os.chdir(cwd)
from oracle import weights as W


def npy(t):
    return t.detach().cpu().numpy()


# the probes of make_golden_emcad.py without the ConvBlock heads the single-supervision decoder does not have, plus the first and the last out_head
PROBES = ["conv.0.weight", "backbone.patch_embed1.proj.weight", "backbone.block3.2.attn.kv.weight", "backbone.norm4.weight",
          "decoder.mscb4.0.pconv1.0.weight", "decoder.mscb4.0.msdc.dwconvs.0.0.weight", "decoder.mscb4.0.msdc.dwconvs.2.0.weight", "decoder.mscb4.0.pconv2.0.weight",
          "decoder.mscb4.0.msdc.dwconvs.1.1.weight", "decoder.eucb3.up_dwc.1.weight", "decoder.eucb3.pwc.0.weight", "decoder.eucb3.pwc.0.bias",
          "decoder.lgag3.W_g.0.weight", "decoder.lgag3.W_x.0.bias", "decoder.lgag3.psi.0.weight", "decoder.lgag3.psi.1.weight", "decoder.lgag1.W_x.0.weight",
          "decoder.cab4.fc1.weight", "decoder.cab2.fc2.weight", "decoder.sab.conv.weight", "decoder.mscb1.0.pconv2.1.bias",
          "out_head4.weight", "out_head4.bias", "out_head1.weight", "out_head1.bias"]
NP = 256
SCALES = (32, 16, 8, 4)
W_CE, W_DICE = 0.3, 0.7                                  # trainer.py:143


def build(dtype):
    m = EMCADNet(num_classes=9, kernel_sizes=[1, 3, 5], expansion_factor=2, dw_parallel=True, add=True, lgag_ks=3, activation="relu6",
                 encoder="pvt_v2_b2", pretrain=False)
    assert m.dual is False
    m.backbone.reset_drop_path(0.0)
    return m.to(dtype)


def main(size=64, n=2):
    sys.path.insert(0, REF)
    for missing in ("medpy", "seaborn", "segmentation_mask_overlay", "SimpleITK", "thop", "ptflops"):
        _stub(missing, metric=None, overlay_masks=None, profile=None, clever_format=None, get_model_complexity_info=None)
    cwd = os.getcwd(); os.chdir(REF)
    try:
        from utils.utils import powerset, DiceLoss
    finally:
        os.chdir(cwd)
    man = type(W.manifest_emcadnet(9))((k, v) for k, v in W.manifest_emcadnet(9).items() if not k.startswith("decoder.ConvBlock"))
    model = build(torch.float32)
    ref = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert list(ref.items()) == [(k, list(v)) for k, v in man.items()], "manifest mismatch (EMCADNet, single supervision)"
    json.dump({"emcadnet_single_k9": ref, "n_params": sum(p.numel() for p in model.parameters())}, open(os.path.join(HERE, "manifest_emcad_single.json"), "w"))
    sd0 = W.make_state_dict(man, seed=5)
    model.load_state_dict(sd0, strict=True)
    model.train()
    g = torch.Generator().manual_seed(77)
    x = torch.randn(n, 1, size, size, generator=g)
    label = torch.randint(0, 9, (n, size, size), generator=g)
    # blocky labels (organ-like regions) instead of per-pixel noise - the labels of emcad_64.npz
    label = F.interpolate(label[:, None, ::8, ::8].float(), size=(size, size), mode="nearest")[:, 0].long()
    out = {"x": npy(x), "label": npy(label), "scales": np.asarray(SCALES)}
    out_idxs = list(range(4))
    SS = {"mutation": [s for s in powerset(out_idxs)], "deep_supervision": [[i] for i in out_idxs], "last": [[-1]]}      # trainer.py:113-119

    def run(m, xx, pre):
        heads = {}
        hooks = [getattr(m, f"out_head{lvl}").register_forward_hook(lambda mod, inp, o, i=i: heads.__setitem__(i, o.detach().clone())) for i, lvl in enumerate((4, 3, 2, 1))]
        P = m(xx, mode="train")
        for h in hooks:
            h.remove()
        ce = nn.CrossEntropyLoss(); dl = DiceLoss(9)

        def total(ss):                                        # trainer.py:141-153
            loss = 0.0
            for s in ss:
                if s == []:
                    continue
                iout = 0.0
                for idx in range(len(s)):
                    iout = iout + P[s[idx]]
                loss = loss + (W_CE * ce(iout, label.long()) + W_DICE * dl(iout, label, softmax=True))
            return loss
        with torch.no_grad():
            for mode in ("deep_supervision", "last"):
                out[pre + "loss." + mode] = npy(total(SS[mode]))
        loss = total(SS["mutation"])
        loss.backward()
        out[pre + "loss.mutation"] = npy(loss)
        names = dict(m.named_parameters())
        for i, o in enumerate(P):
            assert torch.equal(F.interpolate(heads[i], scale_factor=SCALES[i], mode="bilinear"), o.detach()), i
            out[f"{pre}head{i}"] = npy(heads[i])
        for k in PROBES:
            out[pre + "graw." + k] = npy(names[k].grad.reshape(-1)[:NP]); out[pre + "grawnorm." + k] = npy(names[k].grad.norm())
        return loss
    loss = run(model, x, "")
    m64 = build(torch.float32); m64.load_state_dict(sd0, strict=True); m64 = m64.double().train()
    l64 = run(m64, x.double(), "f64.")
    path = os.path.join(HERE, "emcad_single_64.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "emcad_64.npz"))
    print("wrote emcad_single_64.npz", len(out), "arrays,", os.path.getsize(path), "bytes; loss", float(loss.detach()), "float64", float(l64.detach()))


if __name__ == "__main__":
    main()
