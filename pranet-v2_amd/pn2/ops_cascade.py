"""Engine ops, part 4: the attention gate of the CASCADE decoders, additive and concatenating (csrc/pn2_cascade.hip).  Mixed into pn2.engine.Engine."""
import ctypes as C

from .capi import call
from .core import Act, _p, _stream, rup
from .ops_conv import _bn_desc


class _GatePsi:
    """What the psi branch of one gate leaves for the apply step and the backward pass (CascadeOps._gate_psi)."""
    __slots__ = ("F", "Fp", "M", "g1", "sg", "hg", "x1", "sx", "hx", "w", "psi_conv", "psi_bn", "psi_raw", "a", "b", "mean", "invstd", "bd")


class CascadeOps:
    def _gate_psi(self, what, g, x, W_g, bn_g, W_x, bn_x, psi_conv, psi_bn):
        """The part of the gate that does not depend on the aggregation: the two deferred 1x1 convs, pn2_ag_psi_fwd and the one-channel BatchNorm rows -> _GatePsi."""
        F = psi_conv.in_channels
        assert (g.N, g.H, g.W, g.C, g.Cp, g.dt) == (x.N, x.H, x.W, x.C, x.Cp, x.dt) and g.dt == self.dt and g.gw == g.C and x.gw == x.C, f"{what}: g and x of one plain layout"
        assert W_g.out_channels == F and W_x.out_channels == F and psi_conv.out_channels == 1 and W_g.kernel_size == (1, 1) and W_x.kernel_size == (1, 1) and psi_conv.kernel_size == (1, 1)
        k = _GatePsi()
        k.F, k.psi_conv, k.psi_bn = F, psi_conv, psi_bn
        Fp, M, dt, st, nul = rup(F, 8), g.M, self.dt, _stream(), C.c_void_p(0)
        k.Fp, k.M = Fp, M
        ops = []
        for a, conv, bn in ((g, W_g, bn_g), (x, W_x, bn_x)):
            o = self.conv_bn_act(a, conv, bn, bias=conv.bias, defer_out="biased")
            d, rows = o.deferred, (None, None)
            if d is not None:          # neither finalized nor written by conv_bn_act: the rows are made here, the output never
                self._bn_forward(d.bn, d.bd, d.par, d.psum, d.psq, d.nblk, d.bias)
                o.deferred, rows = None, (d.scale, d.shift)
            assert o.Cp == Fp
            ops.append((o, rows))
        (g1, (sg, hg)), (x1, (sx, hx)) = ops
        k.g1, k.sg, k.hg, k.x1, k.sx, k.hx = g1, sg, hg, x1, sx, hx
        w = k.w = psi_conv.weight
        psi_raw = k.psi_raw = self.fbuf(M)
        k.mean = k.invstd = k.bd = None
        if self.training:
            nb, rows_blk = call.pn2_ag_blocks(dt, M, Fp, 0), call.pn2_ag_psi_rows(dt, M, Fp)
            if nb < 1 or rows_blk < 1:
                raise RuntimeError(f"{what}: unsupported geometry")
            pm, pq = self.fbuf(nb), self.fbuf(nb)
            call.pn2_ag_psi_fwd(dt, g1.ptr, g1.ld, _p(sg), _p(hg), x1.ptr, x1.ld, _p(sx), _p(hx), _p(w), F, Fp, M, _p(psi_raw), _p(pm), _p(pq), st)
            k.bd = _bn_desc(psi_bn, M, 1, 1, 1, 1, tile_rows=rows_blk)
            k.a, k.b, k.mean, k.invstd = self._bn_forward(psi_bn, k.bd, self.fbuf(4, 1), pm, pq, nb, psi_conv.bias)
        else:
            call.pn2_ag_psi_fwd(dt, g1.ptr, g1.ld, _p(sg), _p(hg), x1.ptr, x1.ld, _p(sx), _p(hx), _p(w), F, Fp, M, _p(psi_raw), nul, nul, st)
            k.a, k.b = self._bn_eval_rows(psi_bn, M, 1, 1, 1, 1, psi_conv.bias)
        return k

    def _gate_bwd_tail(self, k, g, dz, p1, p2, nb1, nb2, st):
        """Behind either bwd_gate kernel: pn2_bn_bwd_finalize of the one-channel BatchNorm, pn2_ag_bwd_sum, the weight and bias sinks, and the one F_int-wide tensor that is
        the incoming gradient of both convs' BatchNorm backward."""
        dt, F, Fp, M, psi_bn, psi_conv, w = self.dt, k.F, k.Fp, k.M, k.psi_bn, k.psi_conv, k.w
        g1, x1 = k.g1, k.x1
        coef, sinks = self.fbuf(3), self._bn_sinks(psi_bn)
        call.pn2_bn_bwd_finalize(_p(p1), _p(p2), nb1, C.byref(k.bd), _p(psi_bn.weight), _p(k.invstd), _p(sinks[0]), _p(sinks[1]), sinks[2], _p(coef), st)
        dsum = self.empty(g.N, g.H, g.W, Fp)
        pw, pb = self.fbuf(nb2, Fp), self.fbuf(nb2)
        call.pn2_ag_bwd_sum(dt, _p(dz), _p(k.psi_raw), _p(k.a), _p(k.mean), _p(k.invstd), _p(coef), g1.ptr, g1.ld, _p(k.sg), _p(k.hg), x1.ptr, x1.ld, _p(k.sx), _p(k.hx), _p(w), F, Fp, M,
                            _p(dsum), Fp, _p(pw), _p(pb), st)
        gw_, wacc = self.pgrads.sink(w)
        self.colsum_finalize(pw, nb2, F, Fp, gw_, wacc)
        gb_, bacc = self.pgrads.sink(psi_conv.bias)
        self.colsum_finalize(pb, nb2, 1, 1, gb_, bacc)
        for o in (g1, x1):          # d relu(g1 + x1) / d g1 = d / d x1: one tensor is the gradient of both BatchNorm outputs
            assert o.grad is None and not o.grad_written
            o.grad = dsum
            o.grad_written = True

    def _gate(self, what, cat, g, x, W_g, bn_g, W_x, bn_x, psi_conv, psi_bn):
        k = self._gate_psi(what, g, x, W_g, bn_g, W_x, bn_x, psi_conv, psi_bn)
        M, dt, st = g.M, self.dt, _stream()
        if cat:
            Cw = 2 * g.C
            y = Act(self, self.empty(g.N, g.H, g.W, Cw), Cw, Cw, Cw, dt)
            call.pn2_ag_apply_cat_fwd(dt, g.ptr, g.ld, x.ptr, x.ld, _p(k.psi_raw), _p(k.a), _p(k.b), y.ptr, y.ld, M, g.C, g.Cp, st)
        else:
            y = Act(self, self.empty(g.N, g.H, g.W, g.Cp), g.C, g.gw, g.gwp, dt)
            call.pn2_ag_apply_fwd(dt, g.ptr, g.ld, x.ptr, x.ld, _p(k.psi_raw), _p(k.a), _p(k.b), y.ptr, y.ld, M, g.C, g.Cp, st)
        bwd_gate = call.pn2_ag_bwd_gate_cat if cat else call.pn2_ag_bwd_gate

        def bwd():
            if not self.training:
                raise RuntimeError("backward through eval-mode BatchNorm is not supported")
            st = _stream()
            gy = y.grad_buf()
            gx, xacc = x.grad_sink() if x.requires_grad else (None, 0)
            gg, gacc = g.grad_sink() if g.requires_grad else (None, 0)
            nb1, nb2 = call.pn2_ag_blocks(dt, M, g.Cp, 1), call.pn2_ag_blocks(dt, M, k.Fp, 2)
            dz, p1, p2 = self.fbuf(M), self.fbuf(nb1), self.fbuf(nb1)
            bwd_gate(dt, _p(gy), gy.stride(2), x.ptr, x.ld, _p(k.psi_raw), _p(k.a), _p(k.b), _p(k.mean), _p(k.invstd), _p(gx), gx.stride(2) if gx is not None else 0, xacc,
                     _p(gg), gg.stride(2) if gg is not None else 0, gacc, _p(dz), _p(p1), _p(p2), M, g.C, g.Cp, st)
            self._gate_bwd_tail(k, g, dz, p1, p2, nb1, nb2, st)
        self.record(bwd)
        return y

    def attention_gate(self, g, x, W_g, bn_g, W_x, bn_x, psi_conv, psi_bn):
        """g + x * sigmoid(BN_psi(psi_conv(relu(BN_g(W_g g) + BN_x(W_x x)))))   - Attention_block and the "aggregate" line behind it (MIST/lib/decoders.py:73-79,246).

        The two biased 1x1 convs run on conv_bn_act with their train-mode BatchNorm outputs deferred: only the raw conv outputs and the BatchNorm rows exist, and
        pn2_ag_psi_fwd forms relu(g1 + x1) in registers.  Launches of the gate itself: psi_fwd, the one-channel pn2_bn_finalize, apply_fwd; backward: bwd_gate,
        pn2_bn_bwd_finalize, bwd_sum - the F_int-wide gradient it writes is the incoming gradient of BOTH convs' BatchNorm backward.  Eval mode: the convs fold their
        BatchNorm (forward only, as everywhere)."""
        return self._gate("attention_gate", False, g, x, W_g, bn_g, W_x, bn_x, psi_conv, psi_bn)

    def attention_gate_cat(self, g, x, W_g, bn_g, W_x, bn_x, psi_conv, psi_bn):
        """cat(x * psi, g) over the channels, psi as in attention_gate   - Attention_block and the "Concat" line behind it (MIST/lib/decoders.py:73-79,163).

        -> an Act of 2 C channels whose row of 2 C is contiguous (what global_pool, chan_stats, sigmoid_gate and the 3x3 conv take).  The same launches as attention_gate with
        pn2_ag_apply_cat_fwd / pn2_ag_bwd_gate_cat in the place of apply_fwd / bwd_gate: g and x are read once and the row of 2 C is written once, where a pixel gate and two
        copies into a concat buffer read and write x * psi and g twice.  C % 8 == 0 (every reference width): the second half of a row then starts on a 16-byte boundary."""
        if g.C % 8 or g.Cp != g.C:
            raise NotImplementedError(f"attention_gate_cat: {g.C} channels - the concatenating gate takes widths that are a multiple of 8 (no pad lanes between the halves)")
        return self._gate("attention_gate_cat", True, g, x, W_g, bn_g, W_x, bn_x, psi_conv, psi_bn)
