"""Golden data for the concatenating CASCADE decoder from the imported reference (multiclass_seg/MIST/lib/decoders.py:121-199) - build container only.  Data only:
  manifest_cascade_cat.json   state_dict keys, order and shapes of CASCADE_Cat at [768,384,192,96] and [512,320,128,64]
  cascade_cat_small.npz       the pyramid of make_golden_cascade.py (N = 2, channels [64,40,24,16] at 2^2, 4^2, 8^2, 16^2, the same input and probe seeds): the outputs
                              of CASCADE_Cat in train mode and in eval mode, fp32 and float64 runs ("cat.out<i>", "f64.cat.out<i>", "eval.cat.out<i>",
                              "f64.eval.cat.out<i>"); the gradients of L = sum_i <out_i, R_i> (R_i: probe_weights, repeated by the test) with respect to the deepest
                              input, the shallowest skip, three gate weights and ConvBlock3.conv.0.weight, the first conv that reads a concatenated row;
                              "bf16.cat.rel": the relative L2 distance to float64 of every train-mode output of the fp32 module under torch.autocast("cpu", bfloat16)
                              - the bf16 yardstick, as in make_golden_bs32.py;
                              "gate.*": one Attention_block(24, 24, 12) in float64, train mode, with the Concat line (cat(AG(g, x), g)): inputs, weights, output,
                              the probe R [2, 48, 8, 8] and the gradients of <out, R> with respect to g, x and every parameter - what tests/cascadecatref.py is held to.
The weights are not stored: oracle.weights.make_state_dict(manifest of the module, seed=SEED).  The generator asserts that the reference's own fp32 run is within 5e-5
of its float64 run on every output (half the literal 1e-4 gate: make_golden_cascade.py)."""
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden_cascade as G          # noqa: E402   (the reference import, the pyramid and the probe generator)
from oracle import weights as W          # noqa: E402

SEED, CH = G.SEED, G.CH
PROBES = G.PROBES + ("ConvBlock3.conv.0.weight",)
TAG = "cat"


def _manifest(m):
    return OrderedDict((k, tuple(v.shape)) for k, v in m.state_dict().items())


def main():
    ref = G.reference()
    man = OrderedDict()
    for ch in ([768, 384, 192, 96], [512, 320, 128, 64]):
        man[f"CASCADE_Cat:{','.join(map(str, ch))}"] = [[k, list(v.shape)] for k, v in ref.CASCADE_Cat(channels=ch).state_dict().items()]
    with open(os.path.join(HERE, "manifest_cascade_cat.json"), "w") as f:
        json.dump(man, f, indent=0)
    xs = G.inputs()
    out = {"x": xs[0].numpy(), "s0": xs[1].numpy(), "s1": xs[2].numpy(), "s2": xs[3].numpy()}
    sd = W.make_state_dict(_manifest(ref.CASCADE_Cat(channels=CH)), seed=SEED)

    def module(dt, train):
        m = ref.CASCADE_Cat(channels=CH)
        m.load_state_dict(sd, strict=True)
        m = m.to(dt)
        return m.train() if train else m.eval()
    for dt, pre in ((torch.float32, ""), (torch.float64, "f64.")):
        m = module(dt, True)
        ins = [t.detach().clone().to(dt).requires_grad_(True) for t in xs]
        outs = m(ins[0], [ins[1], ins[2], ins[3]])
        Rs = G.probe_weights([o.shape for o in outs])
        sum((o * r.to(dt)).sum() for o, r in zip(outs, Rs)).backward()
        for i, o in enumerate(outs):
            out[f"{pre}{TAG}.out{i}"] = o.detach().numpy()
        out[f"{pre}{TAG}.gx"], out[f"{pre}{TAG}.gs2"] = ins[0].grad.numpy(), ins[3].grad.numpy()
        P = dict(m.named_parameters())
        for k in PROBES:
            out[f"{pre}{TAG}.g.{k}"] = P[k].grad.numpy()
        m = module(dt, False)
        with torch.no_grad():
            for i, o in enumerate(m(xs[0].to(dt), [t.to(dt) for t in xs[1:]])):
                out[f"{pre}eval.{TAG}.out{i}"] = o.numpy()
    m = module(torch.float32, True)
    with torch.no_grad(), torch.autocast("cpu", torch.bfloat16):
        ob = [o.float() for o in m(xs[0], [xs[1], xs[2], xs[3]])]
    rel = lambda a, b: float(np.linalg.norm(a.astype(np.float64).ravel() - b.ravel()) / np.linalg.norm(b.ravel()))
    out[f"bf16.{TAG}.rel"] = np.array([rel(o.numpy(), out[f"f64.{TAG}.out{i}"]) for i, o in enumerate(ob)])
    print(TAG, "torch-autocast bf16 rel-L2 per output", ["%.4f" % v for v in out[f"bf16.{TAG}.rel"]])
    for mode in ("", "eval."):
        worst = max(float(np.abs(out[f"{mode}{TAG}.out{i}"].astype(np.float64) - out[f"f64.{mode}{TAG}.out{i}"]).max()) for i in range(4))
        print(TAG, mode or "train.", "reference fp32 vs float64:", worst)
        assert worst <= 5e-5, (mode, worst)
    for k in ("gx", "gs2") + tuple("g." + p for p in PROBES):
        r32, r64 = out[f"{TAG}.{k}"].astype(np.float64), out[f"f64.{TAG}.{k}"]
        err, scale = float(np.abs(r32 - r64).max()), float(np.abs(r64).max())
        print(TAG, k, "reference fp32 gradient vs float64:", err, "the rule allows", 1e-5 * max(scale, 1e-3) + 1e-6)
    # ---- one gate in float64, with the Concat line
    ag = ref.Attention_block(F_g=24, F_l=24, F_int=12)
    ag.load_state_dict(W.make_state_dict(_manifest(ag), seed=SEED + 2), strict=True)
    ag = ag.double().train()
    g_ = torch.Generator().manual_seed(SEED + 3)
    gg, gx = (torch.randn(2, 24, 8, 8, generator=g_, dtype=torch.float64) for _ in range(2))
    gr = torch.randn(2, 48, 8, 8, generator=g_, dtype=torch.float64)
    gg.requires_grad_(True); gx.requires_grad_(True)
    o = torch.cat((ag(g=gg, x=gx), gg), dim=1)
    (o * gr).sum().backward()
    out.update({"gate.g": gg.detach().numpy(), "gate.x": gx.detach().numpy(), "gate.R": gr.numpy(), "gate.out": o.detach().numpy(), "gate.dg": gg.grad.numpy(), "gate.dx": gx.grad.numpy()})
    for k, v in ag.state_dict().items():
        out["gate.p." + k] = v.numpy()
    for k, v in ag.named_parameters():
        out["gate.d." + k] = v.grad.numpy()
    path = os.path.join(HERE, "cascade_cat_small.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "emcad_64.npz"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
