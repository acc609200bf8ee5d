"""The concatenating attention gate, fused against composed: the launches of Engine.attention_gate_cat (pn2_ag_apply_cat_fwd, pn2_ag_bwd_gate_cat) against the launches the
same gate takes when it is put together from the ops that existed before - a pixel gate that writes x * psi and two copies into the concat buffer, and their backward:

    fused      forward   pn2_ag_apply_cat_fwd                                                             4 M C elements   (read g, x; write 2 C)
               backward  pn2_ag_bwd_gate_cat                                                              5 M C            (read dout 2 C, x; write dx, dg)
    composed   forward   pn2_sigmoid, pn2_gate_mul (x * psi), pn2_copy (x * psi -> cat), pn2_copy (g -> cat)    6 M C
               backward  pn2_copy (dcat -> dg), pn2_copy (dcat -> d(x * psi)), pn2_gate_bwd, pn2_sigmoid_bwd, pn2_gate_mul    8 M C

Both are timed twice: "gate" - these launches alone - and "gate+psi" with the psi path both share in front (pn2_ag_psi_fwd) and behind (pn2_ag_bwd_sum).  The one-channel
BatchNorm launches (a few floats each) are left out on both sides, so psi = sigmoid(psi_raw) (a = 1, b = 0); the composition is also spared the reduction of dz and
dz * xhat that pn2_ag_bwd_gate_cat does on the way, which it would need another launch for.  Every variant is one captured graph, replayed `--iters` times between two
device events; fused and composed alternate, `--reps` times, on the same device in the same process.  The two forms are compared on their outputs first.

    python tools/cascade_cat_bench.py [--batch 24] [--size 224] [--iters 200] [--reps 7]

Shapes: the three gates of a [512,320,128,64] decoder: M = batch * (size/16)^2, (size/8)^2, (size/4)^2 with C = 320, 128, 64 (F_int = 128, 64, 32), bf16 and fp32.
Prints one JSON line per shape and storage type: median and fastest time per replay in microseconds, composed / fused, and the achieved bytes per second of the gate
launches from the element counts above (activations only; the working sets here are far below the 256 MiB of last-level cache, so these are not HBM rates)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pranet-v2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch

DT = {"fp32": 0, "bf16": 1}
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class Case:
    def __init__(self, lib, N, HW, Cc, F, dt):
        self.lib, self.N, self.HW, self.M, self.C, self.F, self.dt, self.d = lib, N, HW, N * HW, Cc, F, dt, DT[dt]
        dev, tdt, M = "cuda", TDT[dt], N * HW
        g = torch.Generator().manual_seed(Cc)
        rn = lambda *s: torch.randn(*s, generator=g)
        self.g, self.x, self.dcat = rn(M, Cc).to(dev, tdt), rn(M, Cc).to(dev, tdt), rn(M, 2 * Cc).to(dev, tdt)
        self.rg, self.rx = rn(M, F).to(dev, tdt), rn(M, F).to(dev, tdt)
        self.w = (rn(F) * 0.3).to(dev)
        self.one, self.zero = torch.ones(1, device=dev), torch.zeros(1, device=dev)
        z = lambda *s, t=tdt: torch.zeros(*s, dtype=t, device=dev)
        f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.psi = f(M)
        nb1, nb2 = lib.pn2_ag_blocks(self.d, M, Cc, 1), lib.pn2_ag_blocks(self.d, M, F, 2)
        assert nb1 >= 1 and nb2 >= 1
        # fused
        self.cat_f, self.dx_f, self.dg_f, self.dz_f, self.p1, self.p2 = z(M, 2 * Cc), z(M, Cc), z(M, Cc), f(M), f(nb1), f(nb1)
        # composed
        self.gate, self.xp, self.cat_c, self.dxp, self.dx_c, self.dg_c, self.dgate, self.dz_c = f(M), z(M, Cc), z(M, 2 * Cc), z(M, Cc), z(M, Cc), z(M, Cc), f(M), f(M)
        # shared tail
        self.ds, self.pw, self.pb = z(M, F), f(nb2, F), f(nb2)

    def _ok(self, rc):
        if rc != 0:
            raise RuntimeError(f"launch failed with status {rc}")

    def psi_fwd(self, st):
        nul = C.c_void_p(0)
        self._ok(self.lib.pn2_ag_psi_fwd(self.d, P(self.rg), self.F, nul, nul, P(self.rx), self.F, nul, nul, P(self.w), self.F, self.F, self.M, P(self.psi), nul, nul, st))

    def bwd_sum(self, dz, st):
        nul = C.c_void_p(0)
        self._ok(self.lib.pn2_ag_bwd_sum(self.d, P(dz), P(self.psi), P(self.one), nul, nul, nul, P(self.rg), self.F, nul, nul, P(self.rx), self.F, nul, nul, P(self.w), self.F, self.F, self.M,
                                         P(self.ds), self.F, P(self.pw), P(self.pb), st))

    def fused(self, st, psi_path):
        L, d, M, Cc = self.lib, self.d, self.M, self.C
        if psi_path:
            self.psi_fwd(st)
        self._ok(L.pn2_ag_apply_cat_fwd(d, P(self.g), Cc, P(self.x), Cc, P(self.psi), P(self.one), P(self.zero), P(self.cat_f), 2 * Cc, M, Cc, Cc, st))
        nul = C.c_void_p(0)
        self._ok(L.pn2_ag_bwd_gate_cat(d, P(self.dcat), 2 * Cc, P(self.x), Cc, P(self.psi), P(self.one), P(self.zero), nul, nul, P(self.dx_f), Cc, 0, P(self.dg_f), Cc, 0,
                                       P(self.dz_f), P(self.p1), P(self.p2), M, Cc, Cc, st))
        if psi_path:
            self.bwd_sum(self.dz_f, st)

    def composed(self, st, psi_path):
        L, d, M, Cc, N, HW = self.lib, self.d, self.M, self.C, self.N, self.HW
        left = lambda t: C.c_void_p(t.data_ptr())
        right = lambda t: C.c_void_p(t.data_ptr() + Cc * t.element_size())
        if psi_path:
            self.psi_fwd(st)
        self._ok(L.pn2_sigmoid(0, P(self.psi), 1, 1, P(self.gate), M, st))
        self._ok(L.pn2_gate_mul(d, P(self.x), P(self.gate), P(self.xp), N, HW, Cc, 1, 0, st))
        self._ok(L.pn2_copy(d, P(self.xp), Cc, d, left(self.cat_c), 2 * Cc, M, Cc, 0, st))
        self._ok(L.pn2_copy(d, P(self.g), Cc, d, right(self.cat_c), 2 * Cc, M, Cc, 0, st))
        self._ok(L.pn2_copy(d, right(self.dcat), 2 * Cc, d, P(self.dg_c), Cc, M, Cc, 0, st))
        self._ok(L.pn2_copy(d, left(self.dcat), 2 * Cc, d, P(self.dxp), Cc, M, Cc, 0, st))
        self._ok(L.pn2_gate_bwd(d, P(self.dxp), P(self.x), P(self.dgate), N, HW, Cc, 1, st))
        self._ok(L.pn2_sigmoid_bwd(0, P(self.dgate), P(self.gate), P(self.dz_c), 1, 1, M, 0, st))
        self._ok(L.pn2_gate_mul(d, P(self.dxp), P(self.gate), P(self.dx_c), N, HW, Cc, 1, 0, st))
        if psi_path:
            self.bwd_sum(self.dz_c, st)

    def graph(self, fn, psi_path):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn(C.c_void_p(torch.cuda.current_stream().cuda_stream), psi_path)
        return g

    def bytes_gate(self):
        """(fused, composed) activation bytes of the gate launches, forward + backward"""
        e = self.M * self.C * self.g.element_size()
        return (4 + 5) * e, (6 + 8) * e


def time_graphs(graphs, iters, reps):
    """graphs: {name: CUDAGraph}; alternating; -> {name: [microseconds per replay] * reps}"""
    for g in graphs.values():
        for _ in range(10):
            g.replay()
    torch.cuda.synchronize()
    out = {k: [] for k in graphs}
    for _ in range(reps):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                g.replay()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) * 1e3 / iters)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cascade_cat_bench needs a GPU: there is nothing to time without one")
    from pn2 import capi
    lib = capi.load()
    torch.cuda.set_device(0)
    for dt in ("bf16", "fp32"):
        for div, Cc, F in ((16, 320, 128), (8, 128, 64), (4, 64, 32)):
            HW = (a.size // div) ** 2
            c = Case(lib, a.batch, HW, Cc, F, dt)
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            c.fused(st, True); c.composed(st, True)
            torch.cuda.synchronize()
            diff = {"cat": float((c.cat_f.float() - c.cat_c.float()).abs().max()), "dx": float((c.dx_f.float() - c.dx_c.float()).abs().max()),
                    "dg": float((c.dg_f.float() - c.dg_c.float()).abs().max()), "dz_rel": float((c.dz_f - c.dz_c).abs().max() / c.dz_c.abs().max())}
            graphs = {"fused.gate": c.graph(c.fused, False), "composed.gate": c.graph(c.composed, False),
                      "fused.gate+psi": c.graph(c.fused, True), "composed.gate+psi": c.graph(c.composed, True)}
            ts = time_graphs(graphs, a.iters, a.reps)
            bf, bc = c.bytes_gate()
            med = {k: statistics.median(v) for k, v in ts.items()}
            print(json.dumps({"dtype": dt, "M": c.M, "C": Cc, "F_int": F,
                              "us_median": {k: round(v, 3) for k, v in med.items()}, "us_best": {k: round(min(v), 3) for k, v in ts.items()},
                              "spread": {k: round((max(v) - min(v)) / med[k], 3) for k, v in ts.items()},
                              "composed_over_fused": {"gate": round(med["composed.gate"] / med["fused.gate"], 3), "gate+psi": round(med["composed.gate+psi"] / med["fused.gate+psi"], 3)},
                              "gate_bytes": {"fused": bf, "composed": bc},
                              "gate_GBps": {"fused": round(bf / med["fused.gate"] * 1e-3, 1), "composed": round(bc / med["composed.gate"] * 1e-3, 1)},
                              "max_abs_diff_fused_vs_composed": diff}), flush=True)


if __name__ == "__main__":
    main()
