"""Golden data for the CASCADE decoders from the imported reference (multiclass_seg/MIST/lib/decoders.py) - build container only.  Data only:
  manifest_cascade.json   state_dict keys, order and shapes of CASCADE_Add and CASCADE_Add_dual(num_class=9) at [768,384,192,96] and [512,320,128,64]
  cascade_small.npz       a small pyramid (N = 2, channels [64,40,24,16] at 2^2, 4^2, 8^2, 16^2), the outputs of CASCADE_Add, CASCADE_Add_dual(num_class=4) with and
                          without softmax in train mode, fp32 and float64 runs, and probed gradients of L = sum_i <out_i, R_i> (R_i from the seeded generator
                          cascaderef-side code repeats: probe_weights) with respect to the deepest input, the shallowest skip and three gate weights;
                          the eval-mode outputs of CASCADE_Add_dual (softmax), fp32 and float64; per variant the relative L2 distance to float64 of every
                          train-mode output of the fp32 modules under torch.autocast("cpu", bfloat16) - the bf16 yardstick, as in make_golden_bs32.py;
                          "gate.*": one Attention_block(24, 24, 12) in float64, train mode, with the aggregate line (g + AG(g, x)): inputs, weights, output,
                          the probe R and the gradients of <out, R> with respect to g, x and every parameter - what tests/cascaderef.py is held to.
The weights are not stored: oracle.weights.make_state_dict(manifest of the module, seed=SEED).  The narrowest stage has 16 channels, not fewer: the reference's
ChannelAttention builds a bottleneck of in_planes // 16 channels, and its forward raises on an empty one.  The generator asserts that the reference's own fp32 run is
within 5e-5 of its float64 run on every output - half the literal 1e-4 gate, so that two fp32 implementations that are each that close to float64 still meet it
(the regime make_golden_cond.py establishes for the residual networks holds here without re-scaling: the decoder has no residual chain)."""
import importlib.util
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _ref_import          # noqa: F401,E402   (the stubs; the decoder file itself needs torch only)
from oracle import weights as W          # noqa: E402

REF_FILE = "/root/reference/multiclass_seg/MIST/lib/decoders.py"
SEED, CH, K, N = 9, [64, 40, 24, 16], 4, 2
PROBES = ("AG1.psi.0.weight", "AG1.W_g.0.weight", "AG3.W_x.0.weight")
VARIANTS = (("add", {}), ("dual_sm", {"num_class": K, "use_softmax": True}), ("dual_nosm", {"num_class": K, "use_softmax": False}))


def reference():
    spec = importlib.util.spec_from_file_location("mist_decoders", REF_FILE)
    mod = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    spec.loader.exec_module(mod)
    return mod


def inputs():
    g = torch.Generator().manual_seed(SEED)
    return [torch.randn(N, c, 2 << i, 2 << i, generator=g) for i, c in enumerate(CH)]


def probe_weights(shapes):
    g = torch.Generator().manual_seed(SEED + 1)
    return [torch.randn(*s, generator=g) for s in shapes]


def main():
    ref = reference()
    man = OrderedDict()
    for ch in ([768, 384, 192, 96], [512, 320, 128, 64]):
        for name, m in (("CASCADE_Add", ref.CASCADE_Add(channels=ch)), ("CASCADE_Add_dual", ref.CASCADE_Add_dual(channels=ch, num_class=9, use_softmax=True))):
            man[f"{name}:{','.join(map(str, ch))}"] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    with open(os.path.join(HERE, "manifest_cascade.json"), "w") as f:
        json.dump(man, f, indent=0)
    xs = inputs()
    out = {"x": xs[0].numpy(), "s0": xs[1].numpy(), "s1": xs[2].numpy(), "s2": xs[3].numpy()}
    for tag, kw in VARIANTS:
        cls = ref.CASCADE_Add_dual if kw else ref.CASCADE_Add
        m32 = cls(channels=CH, **kw)
        sd = W.make_state_dict(OrderedDict((k, tuple(v.shape)) for k, v in m32.state_dict().items()), seed=SEED)
        worst = 0.0
        for dt, pre in ((torch.float32, ""), (torch.float64, "f64.")):
            m = cls(channels=CH, **kw)
            m.load_state_dict(sd, strict=True)
            m = m.to(dt).train()
            ins = [t.detach().clone().to(dt).requires_grad_(True) for t in xs]
            outs = m(ins[0], [ins[1], ins[2], ins[3]])
            Rs = probe_weights([o.shape for o in outs])
            L = sum((o * r.to(dt)).sum() for o, r in zip(outs, Rs))
            L.backward()
            for i, o in enumerate(outs):
                out[f"{pre}{tag}.out{i}"] = o.detach().numpy()
            out[f"{pre}{tag}.gx"], out[f"{pre}{tag}.gs2"] = ins[0].grad.numpy(), ins[3].grad.numpy()
            P = dict(m.named_parameters())
            for k in PROBES:
                out[f"{pre}{tag}.g.{k}"] = P[k].grad.numpy()
        m = cls(channels=CH, **kw)
        m.load_state_dict(sd, strict=True)
        m.train()
        with torch.no_grad(), torch.autocast("cpu", torch.bfloat16):
            ob = [o.float() for o in m(xs[0], [xs[1], xs[2], xs[3]])]
        rel = lambda a, b: float(np.linalg.norm(a.astype(np.float64).ravel() - b.ravel()) / np.linalg.norm(b.ravel()))
        out[f"bf16.{tag}.rel"] = np.array([rel(o.numpy(), out[f"f64.{tag}.out{i}"]) for i, o in enumerate(ob)])
        print(tag, "torch-autocast bf16 rel-L2 per output", ["%.4f" % v for v in out[f"bf16.{tag}.rel"]])
        if tag == "dual_sm":
            for dt, pre in ((torch.float32, ""), (torch.float64, "f64.")):
                m = cls(channels=CH, **kw)
                m.load_state_dict(sd, strict=True)
                m = m.to(dt).eval()
                with torch.no_grad():
                    for i, o in enumerate(m(xs[0].to(dt), [t.to(dt) for t in xs[1:]])):
                        out[f"{pre}eval.{tag}.out{i}"] = o.numpy()
        for i in range(len(outs)):
            worst = max(worst, float(np.abs(out[f"{tag}.out{i}"].astype(np.float64) - out[f"f64.{tag}.out{i}"]).max()))
        print(tag, "outputs", len(outs), "reference fp32 vs float64:", worst)
        assert worst <= 5e-5, (tag, worst)
    # ---- one gate in float64
    ag = ref.Attention_block(F_g=24, F_l=24, F_int=12)
    ag.load_state_dict(W.make_state_dict(OrderedDict((k, tuple(v.shape)) for k, v in ag.state_dict().items()), seed=SEED + 2), strict=True)
    ag = ag.double().train()
    g_ = torch.Generator().manual_seed(SEED + 3)
    gg, gx, gr = (torch.randn(2, 24, 8, 8, generator=g_, dtype=torch.float64) for _ in range(3))
    gg.requires_grad_(True); gx.requires_grad_(True)
    o = gg + ag(g=gg, x=gx)
    (o * gr).sum().backward()
    out.update({"gate.g": gg.detach().numpy(), "gate.x": gx.detach().numpy(), "gate.R": gr.numpy(), "gate.out": o.detach().numpy(), "gate.dg": gg.grad.numpy(), "gate.dx": gx.grad.numpy()})
    for k, v in ag.state_dict().items():
        out["gate.p." + k] = v.numpy()
    for k, v in ag.named_parameters():
        out["gate.d." + k] = v.grad.numpy()
    path = os.path.join(HERE, "cascade_small.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "emcad_64.npz"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
