"""Launch trace of the C ABI, to compare two trees that share one library (a host-side refactor must leave it unchanged): every launching entry point (the non-value
entries of capi.SIGNATURES, hooked like pn2.profile.Recorder does) becomes one line with all its arguments - numbers as they are, structs passed by pointer with all
their non-pointer fields, every pointer as the index of its first appearance in the run (0 = null), so traces compare across processes.

    PN2_LIB=<libpn2_hip.so> python tools/launch_trace.py --root <tree> --model v2 --dtype bf16,fp32 --out trace.txt [--eval] [--sweep SPLITK=False,...] [--state s.pt]"""
import argparse
import ctypes as C
import importlib
import os
import sys

os.environ.setdefault("PN2_NO_PRETRAINED", "1")
MODELS = ("v2", "v1", "pvt_v2", "emcad_b2", "emcad_b0")


def hook(capi, lines, ids):

    def ptr(v):
        v = (v.value if isinstance(v, C.c_void_p) else v) or 0
        return ids.setdefault(v, len(ids) + 1) if v else 0

    def fmt(v, ct=None):
        if isinstance(v, C.Structure):
            return "{" + " ".join(f"{n}={fmt(getattr(v, n), t)}" for n, t in v._fields_) + "}"
        if isinstance(v, C.Array):
            return "[" + " ".join(fmt(e, v._type_) for e in v) + "]"
        if ct is C.c_void_p or isinstance(v, C.c_void_p):
            return f"@{ptr(v)}"
        if hasattr(v, "_obj"):          # byref(struct)
            return fmt(v._obj)
        return "@0" if v is None else repr(v.value if hasattr(v, "value") else v)
    lib = capi.load()
    for name, argtypes in capi.SIGNATURES.items():
        if name in capi._VALUE_FUNCS:
            continue

        def wrapped(*a, _fn=getattr(lib, name), _name=name, _types=argtypes):
            lines.append(_name + " " + " ".join(fmt(v, t) for v, t in zip(a, _types)))
            rc = _fn(*a)
            if rc != 0:
                raise RuntimeError(f"{_name} failed with status {rc}")
        setattr(capi.call, name, wrapped)


def switch_module(name):
    """the module that holds behaviour switch `name` (tests/test_gpu_switches.py: pn2.core, pn2.lockstep or lib.Res2Net_v1b)"""
    for mod in ("pn2.core", "pn2.lockstep", "lib.Res2Net_v1b"):
        m = importlib.import_module(mod)
        if hasattr(m, name):
            return m
    raise KeyError(name)


def build(name, W):
    import torch
    torch.manual_seed(0)
    if name in ("v2", "pvt_v2"):
        from lib.pranet import PraNet_V2, PVT_PraNet_V2
        m = PraNet_V2(num_class=1) if name == "v2" else PVT_PraNet_V2(num_class=1)
        m.load_state_dict(W.make_state_dict(W.manifest_pranet_v2(1) if name == "v2" else W.manifest_pvt_pranet_v2(1), seed=0), strict=True)
    elif name == "v1":
        from lib.PraNet_Res2Net import PraNet
        m = PraNet()
    else:
        from lib.networks import EMCADNet
        m = EMCADNet(num_classes=9, kernel_sizes=[1, 3, 5], expansion_factor=2, dw_parallel=True, add=True, lgag_ks=3, activation="relu6",
                     encoder="pvt_v2_" + name[-2:], pretrain=False, dual=True)
    if hasattr(m, "backbone") and hasattr(m.backbone, "reset_drop_path"):
        m.backbone.reset_drop_path(0.0)
    return m.cuda()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the tree whose pn2 / lib / oracle packages are traced")
    ap.add_argument("--model", choices=MODELS, default="v2")
    ap.add_argument("--dtype", default="bf16", help="compute dtype, or a comma list: one run each")
    ap.add_argument("--eval", action="store_true", help="one eval-mode forward without gradients instead of training steps")
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--sweep", metavar="NAME=VALUE,...", help="one run per switch, set for that run only; PN2_* names are environment variables")
    ap.add_argument("--out", required=True)
    ap.add_argument("--state", help="torch.save the losses of every step, Trainer.gflat and last_outs here (v2 / pvt_v2 training)")
    ap.add_argument("--save-tuner", help="core.save_tuner to this file at the end, and the tuner's keys (sorted reprs) to <file>.keys")
    a = ap.parse_args()
    sys.path[:0] = [a.root, os.path.join(a.root, "pranet-v2_amd")]
    import torch
    import pn2
    from pn2 import capi, core
    from oracle import weights as W
    x, mask = (t.cuda() for t in W.synthetic_batch(a.batch, a.size, seed=1234))
    lines, ids, state = [], {}, {}
    hook(capi, lines, ids)
    for dt in a.dtype.split(","):
        for sw in a.sweep.split(",") if a.sweep else [None]:          # one run per switch, each set for that run only (PN2_* = environment, else a pn2.core constant)
            ids.clear()
            lines.append(f"# {a.model} {dt} {'eval' if a.eval else 'train'} {sw}")
            k, v = sw.split("=", 1) if sw else ("", "")
            if k.startswith("PN2_"):
                old, os.environ[k] = os.environ.get(k), v
            elif k:
                old = getattr(switch_module(k), k)
                setattr(switch_module(k), k, eval(v))
            pn2.set_compute_dtype(dt)
            model = build(a.model, W)
            if a.eval:
                with torch.no_grad():
                    model.eval()(x)
            elif a.model in ("v2", "pvt_v2"):
                from pn2.trainer import Trainer
                tr = Trainer(model.train(), lr=1e-4, clip=0.5)
                state["loss"] = [tr.step(x, mask).clone() for _ in range(a.steps)]
                state["gflat"], state["outs"] = tr.gflat.clone(), tr.last_outs.clone()
            else:
                outs = model.train()(x, mode="train") if a.model.startswith("emcad") else model.train()(x)
                sum(o.float().square().mean() for o in outs).backward()
            torch.cuda.synchronize()
            if k.startswith("PN2_"):
                os.environ.pop(k) if old is None else os.environ.update({k: old})
            elif k:
                setattr(switch_module(k), k, old)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if a.state:
        torch.save(state, a.state)
    if a.save_tuner:
        core.save_tuner(a.save_tuner)
        with open(a.save_tuner + ".keys", "w") as f:
            f.write("\n".join(sorted(map(repr, core.TUNER))) + "\n")
    print(f"{a.out}: {len(lines)} launches")


if __name__ == "__main__":
    main()
