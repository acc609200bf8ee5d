"""Engine ops, part 4: the additive attention gate of the CASCADE decoders (csrc/pn2_cascade.hip).  Mixed into pn2.engine.Engine."""
import ctypes as C

from .capi import call
from .core import Act, _p, _stream, rup
from .ops_conv import _bn_desc


class CascadeOps:
    def attention_gate(self, g, x, W_g, bn_g, W_x, bn_x, psi_conv, psi_bn):
        """g + x * sigmoid(BN_psi(psi_conv(relu(BN_g(W_g g) + BN_x(W_x x)))))   - Attention_block and the "aggregate" line behind it (MIST/lib/decoders.py:73-79,246).

        The two biased 1x1 convs run on conv_bn_act with their train-mode BatchNorm outputs deferred: only the raw conv outputs and the BatchNorm rows exist, and
        pn2_ag_psi_fwd forms relu(g1 + x1) in registers.  Launches of the gate itself: psi_fwd, the one-channel pn2_bn_finalize, apply_fwd; backward: bwd_gate,
        pn2_bn_bwd_finalize, bwd_sum - the F_int-wide gradient it writes is the incoming gradient of BOTH convs' BatchNorm backward.  Eval mode: the convs fold their
        BatchNorm (forward only, as everywhere)."""
        F = psi_conv.in_channels
        assert (g.N, g.H, g.W, g.C, g.Cp, g.dt) == (x.N, x.H, x.W, x.C, x.Cp, x.dt) and g.dt == self.dt and g.gw == g.C and x.gw == x.C, "attention_gate: g and x of one plain layout"
        assert W_g.out_channels == F and W_x.out_channels == F and psi_conv.out_channels == 1 and W_g.kernel_size == (1, 1) and W_x.kernel_size == (1, 1) and psi_conv.kernel_size == (1, 1)
        Fp, M, dt, st, nul = rup(F, 8), g.M, self.dt, _stream(), C.c_void_p(0)
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
        w = psi_conv.weight
        psi_raw = self.fbuf(M)
        if self.training:
            nb, rows_blk = call.pn2_ag_blocks(dt, M, Fp, 0), call.pn2_ag_psi_rows(dt, M, Fp)
            if nb < 1 or rows_blk < 1:
                raise RuntimeError("attention_gate: unsupported geometry")
            pm, pq = self.fbuf(nb), self.fbuf(nb)
            call.pn2_ag_psi_fwd(dt, g1.ptr, g1.ld, _p(sg), _p(hg), x1.ptr, x1.ld, _p(sx), _p(hx), _p(w), F, Fp, M, _p(psi_raw), _p(pm), _p(pq), st)
            bd = _bn_desc(psi_bn, M, 1, 1, 1, 1, tile_rows=rows_blk)
            a_, b_, mean, invstd = self._bn_forward(psi_bn, bd, self.fbuf(4, 1), pm, pq, nb, psi_conv.bias)
        else:
            call.pn2_ag_psi_fwd(dt, g1.ptr, g1.ld, _p(sg), _p(hg), x1.ptr, x1.ld, _p(sx), _p(hx), _p(w), F, Fp, M, _p(psi_raw), nul, nul, st)
            a_, b_ = self._bn_eval_rows(psi_bn, M, 1, 1, 1, 1, psi_conv.bias)
        y = Act(self, self.empty(g.N, g.H, g.W, g.Cp), g.C, g.gw, g.gwp, dt)
        call.pn2_ag_apply_fwd(dt, g.ptr, g.ld, x.ptr, x.ld, _p(psi_raw), _p(a_), _p(b_), y.ptr, y.ld, M, g.C, g.Cp, st)

        def bwd():
            if not self.training:
                raise RuntimeError("backward through eval-mode BatchNorm is not supported")
            st = _stream()
            gy = y.grad_buf()
            gx, xacc = x.grad_sink() if x.requires_grad else (None, 0)
            gg, gacc = g.grad_sink() if g.requires_grad else (None, 0)
            nb1, nb2 = call.pn2_ag_blocks(dt, M, g.Cp, 1), call.pn2_ag_blocks(dt, M, Fp, 2)
            dz, p1, p2 = self.fbuf(M), self.fbuf(nb1), self.fbuf(nb1)
            call.pn2_ag_bwd_gate(dt, _p(gy), gy.stride(2), x.ptr, x.ld, _p(psi_raw), _p(a_), _p(b_), _p(mean), _p(invstd), _p(gx), gx.stride(2) if gx is not None else 0, xacc,
                                 _p(gg), gg.stride(2) if gg is not None else 0, gacc, _p(dz), _p(p1), _p(p2), M, g.C, g.Cp, st)
            coef, sinks = self.fbuf(3), self._bn_sinks(psi_bn)
            call.pn2_bn_bwd_finalize(_p(p1), _p(p2), nb1, C.byref(bd), _p(psi_bn.weight), _p(invstd), _p(sinks[0]), _p(sinks[1]), sinks[2], _p(coef), st)
            dsum = self.empty(g.N, g.H, g.W, Fp)
            pw, pb = self.fbuf(nb2, Fp), self.fbuf(nb2)
            call.pn2_ag_bwd_sum(dt, _p(dz), _p(psi_raw), _p(a_), _p(mean), _p(invstd), _p(coef), g1.ptr, g1.ld, _p(sg), _p(hg), x1.ptr, x1.ld, _p(sx), _p(hx), _p(w), F, Fp, M,
                                _p(dsum), Fp, _p(pw), _p(pb), st)
            gw_, wacc = self.pgrads.sink(w)
            self.colsum_finalize(pw, nb2, F, Fp, gw_, wacc)
            gb_, bacc = self.pgrads.sink(psi_conv.bias)
            self.colsum_finalize(pb, nb2, 1, 1, gb_, bacc)
            for o in (g1, x1):          # d relu(g1 + x1) / d g1 = d / d x1: one tensor is the gradient of both BatchNorm outputs
                assert o.grad is None and not o.grad_written
                o.grad = dsum
                o.grad_written = True
        self.record(bwd)
        return y
