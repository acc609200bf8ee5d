"""Engine ops, part 1: weight packing, the per-shape kernel / tile tuners, conv (+ BatchNorm + activation + residual) forward and backward, the
fused multi-conv GEMM, deferred column sums, nn.Linear.  Mixed into pn2.engine.Engine; the behaviour switches are read from pn2.core at call time.

Module level: the descriptor builders (_conv_desc, _wgrad_desc, _bn_desc, _relu_code), the wgrad split heuristic (_wgrad_splits), the tuners' timing loop (_time_candidates).
ConvOps.conv_bn_act is an orchestrator over named steps that share one per-call record (_conv_geometry): _conv_eval_fused, _conv_fwd_gemm, _bn_forward, _conv_output; its
backward _conv_bwd: _bwd_incoming, _bn_backward_quad / _bn_backward_segs / _bn_backward_plain or _bwd_no_bn, _bwd_gate, _wgrad, then _dgrad_patch, _dgrad_small_cin or
_dgrad_gemm (_ep_describe, _dgrad_ep).  _bn_forward, _bn_backward_plain, _wgrad: the one BatchNorm / weight-gradient path, also of conv_bn_multi and EncoderOps.bn_after."""
import ctypes as C
from functools import partial
from types import SimpleNamespace

import torch

from . import capi
from . import core
from .capi import call, F32, BF16, F32F, F32X3
from .core import (Act, Bnb, KSPLIT_MINK, TUNE_REPS, WGRAD_SLAB_MB, WGRAD_WGS, _LinearAsConv, _job_table, _p, _stream, _thrash, _w4, rup)

KS_UNTUNED = 3 | (1 << 2) | (2 << 4) | 0x40          # tuning code: LDS-DMA 2-stage ring, 64 x 128 tile, two K groups (see ConvOps._untuned)
_MMA_KEY = {F32F: "f32f", F32X3: "f32x3"}           # tuner-key suffix of the fp32-storage modes whose register-staged tiles are tuned per shape

def _relu_code(relu):
    """relu: False / True (ReLU) / 2 (ReLU6) -> the activation code of the affine passes."""
    return (2 if relu == 2 else 1) if relu else 0


def _conv_desc(N, H, W, OH, OW, Cin_p, ld_in, Cout, ld_out, k=(1, 1, 1, 0, 0, 1, 1), transposed=0, Kp=0, flags=0):
    """capi.ConvDesc; k = (KH, KW, stride, pad_h, pad_w, dil_h, dil_w), default: 1x1, stride 1."""
    d = capi.ConvDesc()
    d.N, d.H, d.W, d.OH, d.OW = N, H, W, OH, OW
    d.Cin_p, d.ld_in, d.Cout, d.ld_out = Cin_p, ld_in, Cout, ld_out
    d.KH, d.KW, d.stride, d.pad_h, d.pad_w, d.dil_h, d.dil_w = k
    d.transposed, d.Kp, d.flags = transposed, Kp, flags
    return d


def _wgrad_desc(N, H, W, OH, OW, Cin_p, ld_x, Cout_p, k, Kp):
    """-> (capi.WgradDesc of a dense [M][Cout_p] output gradient against x, the output-channel tile the library takes for it); k as in _conv_desc."""
    d = capi.WgradDesc()
    d.N, d.H, d.W, d.OH, d.OW = N, H, W, OH, OW
    d.Cin_p, d.ld_x, d.Cout_p, d.ld_dy = Cin_p, ld_x, Cout_p, Cout_p
    d.KH, d.KW, d.stride, d.pad_h, d.pad_w, d.dil_h, d.dil_w = k
    tco = call.pn2_wgrad_tile_co(Cout_p)
    d.Rp, d.Kp = rup(Cout_p, tco), Kp
    return d, tco


def _wgrad_splits(M, wd, tco):
    """pixel splits: enough workgroups to fill 256 CUs twice, >= 4 steps each, slabs capped at 24 MB"""
    tiles = (wd.Rp // tco) * (wd.Kp // 128)
    steps = (M + 31) // 32
    return max(1, min(steps // 4 if steps >= 8 else 1, (WGRAD_WGS + tiles - 1) // tiles, (WGRAD_SLAB_MB << 20) // (wd.Rp * wd.Kp * 4) or 1))


def _bn_desc(bn, M, Cp, C_, gw, gwp, ldp=0, tile_rows=0):
    """capi.BnDesc of `bn` over M rows of Cp physical / C_ logical channels in groups of gw padded to gwp; ldp: row stride of partial sums that are a slice of wider rows; tile_rows: rows per partial block (0: raw moments)."""
    d = capi.BnDesc()
    d.M, d.Cp, d.C, d.gw, d.gwp, d.eps, d.momentum = M, Cp, C_, gw, gwp, bn.eps, (bn.momentum if bn.momentum is not None else 0.1)
    d.ldp, d.tile_rows = ldp, tile_rows
    return d


def _time_candidates(cands, run, admit=None):
    """The tuners' timing loop -> the fastest candidate or None.  Per candidate: a warm launch (admit(c, admitted so far), False turns it down; default run(c)), then TUNE_REPS timed run(c); the minimum counts."""
    kept, evs = [], []
    for c in cands:
        if admit is None:
            run(c)
        elif not admit(c, kept):
            continue
        kept.append(c)
        per = []
        for _ in range(TUNE_REPS):
            if core.TUNE_COLD:       # inside a step every conv runs once, on operands the caches have mostly lost (the deferred wgrads run long after dy / x were produced): time it that way
                _thrash()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(c)
            e1.record()
            per.append((e0, e1))
        evs.append(per)
    torch.cuda.synchronize()
    times = [min(a.elapsed_time(b) for a, b in per) for per in evs]
    return kept[min(range(len(kept)), key=lambda i: times[i])] if kept else None


def out_ok_for_dual(eng, s, residual, out, y_dt, y_C, bias, sum_with, gate, tee, pool):
    """Whether the output pass of the conv_bn_act call `s` is the plain same-dtype 16-byte-row pass that pn2_affine_act_dual replaces (residual: the deferred BatchNorm output)."""
    return (core.DUAL_AFFINE and y_C is None and y_dt in (None, eng.dt) and bias is None and sum_with is None and gate is None and tee is None and not pool
            and (residual.N, residual.H, residual.W, residual.Cp, residual.dt) == (s.N, s.OH, s.OW, s.Cp, eng.dt) and s.Cp % s.V == 0
            and (out is None or out.ld % s.V == 0))


class ConvOps:
    # ------------------------------------------------------------------ weights
    def _pack_desc(self, w, x_map, out_map, transposed):
        Cout, Cin, KH, KW = _w4(w)
        gw_in, gwp_in, Cin_p = x_map
        gw_out, gwp_out, Cout_p = out_map
        d = capi.PackDesc()
        d.Cout, d.Cin, d.KH, d.KW = Cout, Cin, KH, KW
        d.Cout_p, d.gw_out, d.gwp_out = Cout_p, gw_out, gwp_out
        d.Cin_p, d.gw_in, d.gwp_in = Cin_p, gw_in, gwp_in
        d.transposed = 1 if transposed else 0
        if transposed:
            d.Rp, d.Kp = rup(Cin_p, 128), rup(KH * KW * Cout_p, 128)
        else:
            d.Rp, d.Kp = rup(Cout_p, 128), rup(KH * KW * Cin_p, 128)
        return d

    def pack(self, w, x_map, out_map, transposed):
        """K-contiguous weight panel in the compute dtype.  With a pack cache (trainer) the panel is persistent and is
        refreshed for ALL convs by one pn2_pack_weights_multi launch per step instead of one launch per conv."""
        cache = self.pack_cache
        key = (id(w), bool(transposed), x_map, out_map, self.dt)
        if cache is not None and key in cache.entries:
            return cache.entries[key]
        d = self._pack_desc(w, x_map, out_map, transposed)
        wp = torch.empty((d.Rp, d.Kp), dtype=self.tdt, device=self.dev)
        call.pn2_pack_weight(self.dt, _p(w), _p(wp), C.byref(d), _stream())
        if cache is not None:
            cache.add(key, w, wp, d)
        return wp, d

    # ------------------------------------------------------------------ per-shape kernel / tile selection
    def _tune_gemm(self, cd, in_ptr, wp, M, Cout, ep=None):
        """Pick (kernel, BM, BN) for this forward/dgrad shape by timing every candidate once (first eager step; results are cached in
        self.tuner and reused under hipGraph capture).  Returns the code for pn2_conv_desc.flags bits 8..15 (0 = library heuristic).
        ep: the launch carries a BatchNorm-backward epilogue (pn2_conv_gemm_ep): the candidates are timed WITH it (its extra operand reads and
        per-tile work favour other tiles than the plain kernel), writing to scratch destinations."""
        fast = self.mma in (F32F, F32X3)                             # fp32fast / fp32x3: tiles of the register-staged kernel are tuned per shape too (64-row tiles win where
        if self.dt != BF16 and not fast:                             # the heuristic takes 128: more workgroups per CU; 716 -> 748 images/s with 64 rows everywhere)
            return 0
        t = self.tuner
        if t is None:                    # PN2_AUTOTUNE=0: the library's heuristic tile, inside the class the shape rule names
            return self._untuned(cd, M, Cout, ep)
        key = ("g", cd.N, cd.H, cd.W, cd.OH, cd.OW, cd.Cin_p, cd.ld_in, Cout, cd.KH, cd.KW, cd.stride, cd.pad_h, cd.pad_w, cd.dil_h, cd.dil_w, cd.transposed)
        if ep is not None:
            key = key + ("ep", ep.a.mode, ep.b.mode, 1 if ep.b.out else 0, cd.flags & capi.CONV_ACCUM) + (("pool",) if ep.pool else ())
        if fast:
            key = key + (_MMA_KEY[self.mma],)
        if key in t:
            if core.TUNE_LOG is not None:
                core.TUNE_LOG.append((key, t[key], "hit"))
            return t[key]
        if torch.cuda.is_current_stream_capturing():
            return self._untuned(cd, M, Cout, ep)
        from . import lockstep as LS
        with LS.pause():                 # the candidates are timed with real launches even inside a lock-step region
            return self._tune_gemm_run(t, key, cd, in_ptr, wp, M, Cout, ep)

    @staticmethod
    def _ks_class(cd, M, Cout):
        """The shape rule of the intra-workgroup split-K kernels (see _tune_gemm_run): about one wave of tiles and a long K loop, no global split-K."""
        ksteps = -(-(cd.KH * cd.KW * cd.Cin_p) // 64)
        return bool(core.KS2 and Cout > 32 and ksteps >= 9 and -(-M // 64) * -(-Cout // 64) <= 484 and not (cd.flags >> 16) & 15)

    def _untuned(self, cd, M, Cout, ep):
        """Tuning code without a timing run (PN2_AUTOTUNE=0, or a shape first met under capture).  The split-K class sums in its own fp32 order, so the
        rule has to hold here too: module eval without the tuner and a tuned Predictor must return the same bits.  2-stage ring, 64 x 128 tile: fits
        the LDS for every shape of the class.  Launches with a BatchNorm-backward epilogue (training only) keep the heuristic: whether a split-K tile
        fits next to their operand tiles is only known by trying, which is the tuner's job."""
        if ep is None and self.dt == BF16 and self._ks_class(cd, M, Cout):
            return KS_UNTUNED
        return 0

    def _tune_gemm_run(self, t, key, cd, in_ptr, wp, M, Cout, ep):
        st = _stream()
        nul = C.c_void_p(0)
        scratch = torch.empty((M, Cout), dtype=self.tdt, device=self.dev)
        d2 = capi.ConvDesc()
        C.memmove(C.byref(d2), C.byref(cd), C.sizeof(capi.ConvDesc))
        d2.ld_out, d2.Cout = Cout, Cout
        if ep is not None:
            d2.flags = cd.flags & capi.CONV_ACCUM
            e2 = capi.ConvEp()
            C.memmove(C.byref(e2), C.byref(ep), C.sizeof(capi.ConvEp))
            nb64 = (M + 63) // 64
            tp = torch.empty((4, nb64, Cout), dtype=torch.float32, device=self.dev)
            e2.a.p1, e2.a.p2, e2.a.ldp = tp[0].data_ptr(), tp[1].data_ptr(), Cout
            if ep.b.out:
                scratch_b = torch.empty((M, Cout), dtype=self.tdt, device=self.dev)
                e2.b.out, e2.b.ld_out = scratch_b.data_ptr(), Cout
                e2.b.p1, e2.b.p2, e2.b.ldp = tp[2].data_ptr(), tp[3].data_ptr(), Cout
            base = d2.flags

            def launch(code):
                d2.flags = base | (code << 8)
                call.pn2_conv_gemm_ep(self.mma, in_ptr, _p(wp), _p(scratch), C.byref(d2), C.byref(e2), st)
        else:
            def launch(code):
                d2.flags = code << 8
                call.pn2_conv_gemm(self.mma, in_ptr, _p(wp), _p(scratch), nul, nul, C.byref(d2), st)
        # Intra-workgroup split-K (conv_dma_gemm_ks, tuning-code bit 6: two K groups of four waves) sums a tile's K loop in another fp32 order than the plain
        # kernels, which all agree bit for bit.  Whether a shape takes it is therefore a RULE of the shape, not of a timing: about one wave of tiles and a long
        # K loop (what the free tuning run of round 5 picked it for) - every call site that computes the same conv gets the same bits, and the tuner chooses
        # kernel / tile inside the class.
        ks2 = self.dt == BF16 and self._ks_class(cd, M, Cout)
        cands, plain = [], []
        for kern in ((1, 2, 3) if self.dt == BF16 else (1,)):             # 1 register-staged, 2 LDS-DMA with a 3-stage ring, 3 LDS-DMA with a 2-stage ring (more workgroups per CU); fp32fast: 1
            for bm in (1, 2):
                if bm == 2 and M <= 64:
                    continue
                for bn in ((1, 2, 3) if self.dt == BF16 else (1, 2)):
                    if (bn == 2 and Cout <= 32) or (bn == 3 and Cout <= 64):
                        continue
                    plain.append(kern | (bm << 2) | (bn << 4))
                    if ks2 and kern >= 2 and bn >= 2 and not (kern == 2 and bm == 2 and bn == 3):          # (128 x 128 with two 3-stage rings: 192 KB)
                        cands.append(kern | (bm << 2) | (bn << 4) | 0x40)

        def admit(code, feasible):
            if ks2 and feasible and not code & 0x40:
                return False          # (the plain kernels only stand in when no split-K tile fits the LDS next to this launch's epilogue operands)
            try:
                launch(code)
            except RuntimeError as err:       # status -4 only: the epilogue's operand tiles of this tile shape do not fit the LDS; anything else is a real failure
                if "status -4" not in str(err):
                    raise
                return False
            return True
        best = _time_candidates(cands + plain if ks2 else plain, launch, admit)
        if best is None:
            raise RuntimeError(f"no conv kernel candidate could be launched for {key}")
        t[key] = best
        return best

    def _ksplit(self, M, K, Cout_p):
        """Split-K factor for a conv GEMM with M output rows and contraction K (bf16 LDS-DMA kernels only).  Measured on cold operands
        (tools/splitk_micro.py): 4 pays for K >= 4096 with M <= 4096 (5x5, 256 channels, 11x11 maps: 66 -> 49 us); shorter contractions lose
        to the partial-tile traffic."""
        if not core.SPLITK or self.dt != BF16 or K < KSPLIT_MINK or M > 4096 or Cout_p % 8:
            return 1
        return 4

    def _stat_blocks(self, M, Cout, tune):
        bm = (tune >> 2) & 3
        if bm:
            b = 64 if bm == 1 else 128
            return (M + b - 1) // b
        return call.pn2_conv_stat_blocks(M, Cout, self.mma)          # (fp32fast picks its own tiles)

    def _tune_wgrad(self, wd, dy_ptr, x_ptr, rd, nsplit, wshape):
        """-> (kernel code, pixel splits) for this wgrad shape.  Candidates: register-staged / LDS-DMA / LDS-DMA with 128 x 256 tiles x
        {1, 1/2, 1/4, 1/8} of the heuristic split count; each is timed together with the slab reduction its split count implies."""
        t = self.tuner
        fast = self.mma in (F32F, F32X3)          # fp32fast / fp32x3: one kernel, but the pixel-split count is worth timing
        if t is None or (self.dt != BF16 and not fast):
            return 0, nsplit
        key = ("w", wd.N, wd.H, wd.W, wd.OH, wd.OW, wd.Cin_p, wd.ld_x, wd.Cout_p, wd.ld_dy, wd.KH, wd.KW, wd.stride, wd.pad_h, wd.pad_w, wd.dil_h, wd.dil_w, nsplit)
        if fast:
            key = key + (_MMA_KEY[self.mma],)
        if key in t:
            return t[key]
        if torch.cuda.is_current_stream_capturing():
            return 0, nsplit
        from . import lockstep as LS
        with LS.pause():
            return self._tune_wgrad_run(t, key, wd, dy_ptr, x_ptr, rd, nsplit, wshape)

    def _tune_wgrad_run(self, t, key, wd, dy_ptr, x_ptr, rd, nsplit, wshape):
        st = _stream()
        slab = torch.empty((nsplit, wd.Rp, wd.Kp), dtype=torch.float32, device=self.dev)
        gw = torch.empty(tuple(wshape), dtype=torch.float32, device=self.dev)
        codes = (1, 2, 3) if (call.pn2_wgrad_tile_co(wd.Cout_p) == 128 and wd.Kp >= 256) else (1, 2)      # 3: LDS-DMA kernel with 128 x 256 tiles
        if self.dt != BF16:
            codes = (1,)
        cands = [(code, ns) for ns in sorted({max(1, nsplit >> k) for k in range(4)}, reverse=True) for code in codes]

        def run(cand):
            wd.tune, ns = cand
            call.pn2_conv_wgrad(self.mma, dy_ptr, x_ptr, _p(slab), C.byref(wd), ns, st)
            call.pn2_wgrad_reduce(_p(slab), _p(gw), C.byref(rd), ns, 0, st)
        best = t[key] = _time_candidates(cands, run)
        return best

    # ------------------------------------------------------------------ conv (+BN +ReLU +residual): the orchestrator, then its steps in the order they run
    def conv_bn_act(self, x, conv, bn=None, relu=False, residual=None, out=None, out_map=None, y_dt=None, y_C=None, bias=None, sum_with=None,
                    raw_out=None, par_out=None, x_last=False, gate=None, tee=None, pool=False, defer_out=False):
        """y = act(BN(conv(x)) + residual)   — BasicConv2d / Bottle2neck pieces.

        conv: nn.Conv2d (bias-free unless `bias` given), bn: nn.BatchNorm2d or None.
        out: optional destination Act view (writes y into a slice of a concat buffer).
        out_map: (gw, gwp) group-padded layout of the produced channels (default identity).
        y_dt/y_C: fp32 K-channel head outputs (physical raw output stays padded to 8).
        sum_with: an Act of the output's geometry that has no other consumer; returns (y, y + sum_with) - the second tensor (Bottle2neck's
                  sp + spx[i+1]) is written by the same pass and keeps its gradient in sum_with's gradient storage.
        raw_out / par_out: where the raw conv output ([N,OH,OW,Cout_p] view) and the BatchNorm's per-channel rows (scale, shift, mean, invstd:
                  a [4][Cout_p] view) go - channel slices of buffers shared by the convs that write one concat buffer (Engine.concat_bnb).
        gate:     a 1-channel fp32 Act of x's geometry in front of a 1x1 conv: the conv sees (1 - sigmoid(gate)) * x (V1 reverse attention,
                  PraNet_Res2Net.py:153-155).  The per-pixel factor is applied to the GEMM's accumulator rows (pn2_conv_gemm_gated) - the gated copy
                  of x is never written; backward: one pass over (raw, dz) of the conv's OUTPUT width, then plain dgrad / wgrad.
        x_last:   the caller guarantees that this conv's data gradient is the LAST contribution to x's gradient (x's first consumer in forward
                  order).  If x is the output of a train-mode BatchNorm, the dgrad GEMM then takes that BatchNorm's backward statistics in its
                  epilogue (pn2_conv_gemm_ep) and x's producer skips its pn2_bn_bwd_reduce pass.
        defer_out: the caller guarantees that the output is consumed ONLY as the `residual` of one later conv_bn_act (Bottle2neck's downsample branch).  A train-mode
                  BatchNorm output without activation is then not written: the returned Act carries the raw conv output and the BatchNorm's rows (Act.deferred), and the
                  consumer's output pass normalises both operands (pn2_affine_act_dual), behind ONE finalize launch for the two BatchNorms.  Bit-identical to the two passes.
                  defer_out="biased": the same for a biased conv whose consumer is NOT a residual add but an op that finalizes the BatchNorm itself (_bn_forward with the record's
                  bias) and reads raw + rows (CascadeOps.attention_gate).
        """
        assert tee is None or (self.training and bn is not None and bias is None and gate is None and sum_with is None), "tee: train-mode conv + BatchNorm outputs only"
        # pool: the op is conv -> BatchNorm -> ReLU -> MaxPool2d(3, 2, 1) and returns the POOLED activation; the full-resolution BatchNorm output is never written
        # (pn2_bn_relu_maxpool_fwd; backward: pn2_maxpool3x3s2_bwd, then the BatchNorm passes with the mask recomputed from raw).  Train-mode BatchNorm with a plain ReLU only.
        assert not pool or (self.training and bn is not None and relu is True and bias is None and gate is None and sum_with is None and residual is None and out is None
                            and tee is None and y_C is None and y_dt in (None, self.dt)), "pool: train-mode conv + BatchNorm + ReLU only"
        s = self._conv_geometry(x, conv, out_map)
        s.bn, s.relu, s.residual, s.bias, s.sum_with, s.x_last, s.gate, s.tee, s.pool, s.y_C, s.train_bn = bn, relu, residual, bias, sum_with, x_last, gate, tee, pool, y_C, bn is not None and self.training
        s.wp, s.pd = self.pack(s.w, s.x_map, s.o_map, False)
        # a residual whose BatchNorm output was deferred: normalised inside this op's output pass where that pass is the plain same-dtype one, else written first
        s.dual = s.draw_done = None          # draw_done: the gradient of s.raw once the residual consumer's backward has formed it (_bn_backward_dual)
        if residual is not None and residual.deferred is not None:
            if (s.train_bn and out_ok_for_dual(self, s, residual, out, y_dt, y_C, bias, sum_with, gate, tee, pool)):
                s.dual = residual.deferred
            else:
                self._materialize(residual)
        # biased conv / nn.Linear with nothing behind it (no BN, activation, residual or re-layout): the bias goes into the GEMM epilogue and
        # the GEMM writes the output itself - no separate affine pass
        s.fuse_bias = (core.FUSE_BIAS and bn is None and bias is not None and not relu and residual is None and out is None and y_C is None and (y_dt is None or y_dt == self.dt))
        s.bvec = None
        if s.fuse_bias:
            out = self._new_out(s)
            s.raw, s.bvec = out.t, self._padded_bias(bias, s.Cout, s.Cp)
        elif raw_out is not None:
            assert tuple(raw_out.shape) == (s.N, s.OH, s.OW, s.Cp) and raw_out.dtype == self.tdt and raw_out.stride(2) % s.V == 0
            s.raw = raw_out
        else:
            s.raw = self.empty(s.N, s.OH, s.OW, s.Cp)
        s.raw_ld = s.raw.stride(2)
        cd = _conv_desc(s.N, s.H, s.W, s.OH, s.OW, x.Cp, x.ld, s.Cp, s.raw_ld, s.k, 0, s.pd.Kp, capi.CONV_STATS if s.train_bn else 0)
        tune = self._tune_gemm(cd, x.ptr, s.wp, s.M, s.Cp)
        cd.flags |= tune << 8
        if (core.EVAL_FUSE and bn is not None and not self.training and not self.need_grad and gate is None and sum_with is None and y_C is None and not s.fuse_bias
                and (y_dt is None or y_dt == self.dt) and self._ksplit(s.M, s.KH * s.KW * x.Cp, s.Cp) == 1 and relu in (False, True, 2)
                and (residual is None or (residual.dt == self.dt and residual.ld % s.V == 0 and s.Cp % s.V == 0 and (out is None or out.ld % s.V == 0)))):
            return self._conv_eval_fused(s, cd, tune, out)
        self._conv_fwd_gemm(s, cd, tune)
        s.scale = s.shift = s.mean = s.invstd = s.par = s.bd = None
        if bn is not None:
            s.bd = _bn_desc(bn, s.M, s.Cp, s.Cout, s.gw_o, s.gwp_o, tile_rows=s.tile_rows)
            s.par = par_out if par_out is not None else self.fbuf(4, s.Cp)          # rows: scale, shift, mean, invstd
            assert tuple(s.par.shape) == (4, s.Cp) and s.par.stride(1) == 1
            s.defer = bool(defer_out and core.DUAL_AFFINE and s.train_bn and not relu and residual is None and out is None and sum_with is None and tee is None and not pool
                           and gate is None and y_C is None and (bias is None or defer_out == "biased") and y_dt in (None, self.dt) and not s.fuse_bias and s.Cp % s.V == 0 and s.raw_ld % s.V == 0)
            if s.defer:             # neither finalized nor written here: the consumer does both (or _materialize)
                s.scale, s.shift, s.mean, s.invstd = s.par[0], s.par[1], s.par[2], s.par[3]
            elif s.dual is not None:
                # the two BatchNorms' finalize launches depend on their own GEMMs only: one table-driven launch for both (inside a lock-step cache; else one after the other)
                d = s.dual
                s.scale, s.shift, s.mean, s.invstd = self.lockstep("bn.dual", [lambda: self._bn_forward(d.bn, d.bd, d.par, d.psum, d.psq, d.nblk),
                                                                               lambda: self._bn_forward(bn, s.bd, s.par, s.psum, s.psq, s.nblk)])[1]
                residual.deferred = None
            else:
                s.scale, s.shift, s.mean, s.invstd = self._bn_forward(bn, s.bd, s.par, s.psum, s.psq, s.nblk, bias)
        elif bias is not None:
            s.shift = self._padded_bias(bias, s.Cout, s.Cp)
        s.y_dt = self.dt if y_dt is None else y_dt
        if bn is not None and s.defer:
            s.out, s.y2, s.pidx, s.ncopy = Act(self, s.raw, s.Cout, s.gw_o, s.gwp_o, self.dt), None, None, s.Cp
            s.out.deferred = s
        else:
            self._conv_output(s, out)
        if not self.need_grad:
            return s.out if s.y2 is None else (s.out, s.y2)
        # the BatchNorm-backward statistics of this output's gradient can be taken by the dgrad GEMM that completes it (x_last of the consumer)
        out, V = s.out, s.V
        s.bnb_ok = (core.BNB_EPILOGUE and s.train_bn and not s.fuse_bias and y_C is None and s.y_dt == self.dt and relu in (False, True) and out.ld % V == 0 and s.Cp % V == 0 and not pool)
        if s.bnb_ok:
            out.bnb = Bnb(s.raw, s.par, bool(relu), out.t if residual is not None else None)
            if not relu and residual is None:
                out.prod = s          # a residual candidate: see _bn_backward_dual
            if (residual is not None and relu and residual.bnb is not None and not residual.bnb.relu and residual.bnb.ymask is None and residual.bnb.split == 0 and residual.parent is None and residual.Cp == s.Cp):
                out.bnb.res = residual          # (only as this op's residual operand: Bottle2neck's downsample branch)
        self.record(partial(self._conv_bwd, s))
        return s.out if s.y2 is None else (s.out, s.y2)

    def _conv_bwd(self, s):
        """Backward of conv_bn_act: incoming gradient -> BatchNorm backward (or bias only) -> gate -> bias gradient -> weight gradient -> data gradient."""
        x, s.st = s.x, _stream()
        s.out.prod = None          # (the link back to this record has served: no reference cycle survives the backward pass)
        self._bwd_incoming(s)
        if s.train_bn and s.draw_done is not None:
            bias_done = s.bias is None          # (the backward of the op this output was the residual of has formed s.draw, with this BatchNorm's parameter gradients: _bn_backward_dual)
        elif s.train_bn:          # in the form the incoming gradient allows: per pooling quad, on statistics dgrad epilogues left, or plain
            coef, sinks = self.fbuf(3 * s.Cp), self._bn_sinks(s.bn)
            segs = s.out.find_bstats() if (s.bnb_ok and s.dy.stride(2) % s.V == 0) else None
            if s.quad:
                self._bn_backward_quad(s, coef, sinks)
            elif segs is not None and len(segs) <= 4 and any(s_[2] is not None for s_ in segs):
                self._bn_backward_segs(s, segs, coef, sinks)
            else:
                self._bn_backward_plain(s, [(s.bn, s.bd, 0)], s.draw, coef, sinks, partial(self._bwd_residual_sink, s))
            bias_done = s.bias is None
        else:
            bias_done = self._bwd_no_bn(s)
        if s.gate is not None:
            self._bwd_gate(s)
        if not bias_done:                                  # biased conv / nn.Linear: db = column sums of dz (~0 under a train-mode BN)
            gb, gba = self.pgrads.sink(s.bias)
            cp = getattr(s.out, "colparts", None)
            if cp is not None and s.draw is s.dy and cp[2].data_ptr() == s.dy.data_ptr() and tuple(cp[0].shape) == (cp[1], s.Cp):
                self.colsum_finalize(cp[0], cp[1], s.Cout, s.Cp, gb, gba)          # (the consumer's data-gradient kernel left the column sums of this very buffer)
            else:
                self.colsum(s.draw, s.M, s.Cp, s.Cout, gb, gba)
        self._wgrad(s, s.draw, s.pd.Kp, [(s.w, s.o_map, 0)], (id(s.w), x.M))
        if not x.requires_grad:
            return
        plain_maps = s.gw_o == s.gwp_o and x.ld == x.Cp and s.dh == 1 and s.dw == 1
        if core.PATCH_DGRAD and plain_maps and s.KH == s.sh and s.KW == s.sw and s.KH > 1 and s.ph == 0 and s.pw == 0 and x.gw == x.gwp:
            self._dgrad_patch(s)
        elif (core.SMALL_CIN_DGRAD and plain_maps and s.Cin <= 4 and s.sh > 1 and s.ph == s.pw and (x.gw == x.gwp or x.Cp == x.gwp) and s.Cp == s.Cout and s.KH * s.KW * s.Cout * 16 <= 64 * 1024):
            self._dgrad_small_cin(s)
        else:
            self._dgrad_gemm(s)

    def _materialize(self, a):
        """Write the deferred BatchNorm output `a` after all (a consumer whose output pass cannot normalise it on the fly): its finalize and its normalise pass, as conv_bn_act would have run them."""
        d, a.deferred = a.deferred, None
        self._bn_forward(d.bn, d.bd, d.par, d.psum, d.psq, d.nblk)
        a.t = self.empty(d.N, d.OH, d.OW, d.Cp)
        call.pn2_affine_act(self.dt, _p(d.raw), d.raw_ld, self.dt, a.ptr, a.ld, d.M, d.Cp, _p(d.scale), _p(d.shift), C.c_void_p(0), 0, 0, d.st)

    def _conv_geometry(self, x, conv, out_map):
        """-> the per-call record of conv_bn_act: geometry and layouts (Cp: the padded OUTPUT width; k: as _conv_desc takes it; V: elements per 16-byte vector); the steps add what they share (operands, wp / pd, raw, par, out ...)."""
        w = conv.weight
        Cout, Cin, KH, KW = _w4(w)
        (sh, sw), (ph, pw), (dh, dw) = conv.stride, conv.padding, conv.dilation
        assert sh == sw and conv.groups == 1
        assert x.C == Cin, (x.C, Cin)
        N, H, W = x.N, x.H, x.W
        OH = (H + 2 * ph - dh * (KH - 1) - 1) // sh + 1
        OW = (W + 2 * pw - dw * (KW - 1) - 1) // sw + 1
        gw_o, gwp_o = out_map if out_map is not None else (Cout, rup(Cout, 8))
        Cp = (Cout + gw_o - 1) // gw_o * gwp_o
        M = N * OH * OW
        return SimpleNamespace(x=x, w=w, Cout=Cout, Cin=Cin, KH=KH, KW=KW, sh=sh, sw=sw, ph=ph, pw=pw, dh=dh, dw=dw, k=(KH, KW, sh, ph, pw, dh, dw), N=N, H=H, W=W, OH=OH, OW=OW,
                               gw_o=gw_o, gwp_o=gwp_o, Cp=Cp, x_map=(x.gw, x.gwp, x.Cp), o_map=(gw_o, gwp_o, Cp), M=M, st=_stream(), V=4 if self.dt == F32 else 8,
                               flops=2 * M * Cout * Cin * KH * KW, shape=f"{Cin}->{Cout} k{KH}x{KW} s{sh} d{dh} {N}x{OH}x{OW}")

    def _new_out(self, s):
        return Act(self, self.empty(s.N, s.OH, s.OW, s.Cp), s.Cout, s.gw_o, s.gwp_o, self.dt)

    def _conv_eval_fused(self, s, cd, tune, out):
        # eval mode (MyTest_med.py:98-104, the in-training evaluation): the folded BatchNorm, the activation and the residual add ride in the GEMM epilogue -
        # no raw conv output, no separate normalise pass (half the launches and half the activation traffic of the layer)
        residual, relu = s.residual, s.relu
        scale, shift = self._bn_eval_rows(s.bn, s.M, s.Cp, s.Cout, s.gw_o, s.gwp_o, s.bias)
        if out is None:
            out = self._new_out(s)
        assert residual is None or residual.Cp == s.Cp
        cd.ld_out = out.ld
        cd.flags = (tune << 8) | capi.CONV_AFFINE | (capi.CONV_RELU6 if relu == 2 else (capi.CONV_RELU if relu else 0))
        capi.WORK.update(flops=s.flops, tag=":fwd", shape=s.shape)
        call.pn2_conv_gemm_affine(self.mma, s.x.ptr, _p(s.wp), out.ptr, _p(scale), _p(shift), residual.ptr if residual is not None else C.c_void_p(0), residual.ld if residual is not None else 0, C.byref(cd), s.st)
        return out

    def _conv_fwd_gemm(self, s, cd, tune):
        """The forward GEMM into s.raw - gated, global split-K + reduce, with a fused bias, or plain; train-mode BatchNorm: + the s.nblk partial rows s.psum / s.psq (s.tile_rows rows per block, 0 = raw moments)."""
        x, M, Cp, st, train_bn = s.x, s.M, s.Cp, s.st, s.train_bn
        s.psum, s.psq, s.nblk, s.tile_rows = None, None, 0, 0
        if train_bn:
            s.nblk = self._stat_blocks(M, Cp, tune)
            s.tile_rows = self._tile_m(M, Cp, tune)
            s.psum, s.psq = self.fbuf(s.nblk, Cp), self.fbuf(s.nblk, Cp)
        capi.WORK.update(flops=s.flops, tag=":fwd", shape=s.shape)
        ksplit = self._ksplit(M, s.KH * s.KW * x.Cp, Cp)
        if tune & 0xC0:
            ksplit = 1          # the tuner found the intra-workgroup split-K kernel faster than every plain tile: it also replaces the global split-K + reduce pair
        if s.gate is not None:
            gate = s.gate
            assert (s.KH, s.KW, s.sh) == (1, 1, 1) and gate.dt == F32 and gate.C == 1 and gate.M == M and s.bias is None, "the fused gate sits in front of a bias-free 1x1 conv"
            call.pn2_conv_gemm_gated(self.mma, x.ptr, _p(s.wp), _p(s.raw), _p(s.psum), _p(s.psq), C.byref(cd), gate.ptr, st)
        elif ksplit > 1:
            # few output rows, long contraction (the 5x5 convs of the ra4 branch on 11x11 maps): the K loop of every tile is shared by ksplit
            # workgroups that leave fp32 partial tiles; the reduce sums them and takes the BatchNorm statistics / adds the bias
            ws = self.fbuf(ksplit, M, Cp)
            cd.flags = ((2 | (1 << 2) | ((3 if Cp > 64 else 2) << 4)) << 8) | (ksplit << 16)
            if train_bn:
                s.nblk, s.tile_rows = (M + 63) // 64, 0          # the reduce leaves raw moments of 64-row blocks
                s.psum, s.psq = self.fbuf(s.nblk, Cp), self.fbuf(s.nblk, Cp)
            call.pn2_conv_gemm(self.mma, x.ptr, _p(s.wp), _p(s.raw), _p(ws), _p(None), C.byref(cd), st)
            call.pn2_conv_splitk_reduce(self.dt, _p(ws), ksplit, M, Cp, _p(s.raw), s.raw_ld, _p(s.bvec), _p(s.psum), _p(s.psq), 0, st)
        elif s.fuse_bias:
            cd.flags |= capi.CONV_BIAS
            call.pn2_conv_gemm(self.mma, x.ptr, _p(s.wp), _p(s.raw), _p(s.bvec), _p(None), C.byref(cd), st)
        else:
            call.pn2_conv_gemm(self.mma, x.ptr, _p(s.wp), _p(s.raw), _p(s.psum), _p(s.psq), C.byref(cd), st)

    def _bn_forward(self, bn, bd, rows, psum, psq, nblk, bias=None):
        """BatchNorm forward of conv_bn_act, conv_bn_multi and bn_after on rows = (scale, shift, mean, invstd): train mode turns the nblk partial rows psum / psq into batch statistics, eval mode folds the running ones (mean = invstd = None).  -> rows"""
        scale, shift, st = rows[0], rows[1], _stream()
        if not self.training:
            call.pn2_bn_eval_prepare(C.byref(bd), _p(bn.weight), _p(bn.bias), _p(bn.running_mean), _p(bn.running_var), _p(scale), _p(shift), st)
            if bias is not None:
                shift[:bd.C] += bias.detach() * scale[:bd.C]
            return scale, shift, None, None
        mean, invstd = rows[2], rows[3]
        call.pn2_bn_finalize(_p(psum), _p(psq), nblk, C.byref(bd), _p(bn.weight), _p(bn.bias), _p(bn.running_mean), _p(bn.running_var), _p(scale), _p(shift), _p(mean), _p(invstd), st)
        self.bn_modules.append(bn)
        if bias is not None:          # biased conv followed by train-mode BN: the output is unchanged, only the running mean sees the bias
            with torch.no_grad():
                bn.running_mean.add_(bias.detach(), alpha=bd.momentum)
        return scale, shift, mean, invstd

    def _conv_output(self, s, out):
        """The pass from raw to the output(s): pooled, the sum_with pair, tee'd, or plain (none with a fused bias).  Sets s.out, s.y2 (None without sum_with), s.pidx (the pool's argmax bytes), s.ncopy."""
        N, OH, OW, Cp, M, V, st = s.N, s.OH, s.OW, s.Cp, s.M, s.V, s.st
        residual, sum_with, tee, y_dt, y_C, raw, raw_ld = s.residual, s.sum_with, s.tee, s.y_dt, s.y_C, s.raw, s.raw_ld
        s.pidx = s.y2 = None
        if s.pool:
            PH, PW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
            out = Act(self, self.empty(N, PH, PW, Cp), s.Cout, s.gw_o, s.gwp_o, self.dt)
            s.pidx = self.alloc((N, PH, PW, Cp), torch.uint8)
            call.pn2_bn_relu_maxpool_fwd(self.dt, _p(raw), raw_ld, _p(s.scale), _p(s.shift), out.ptr, out.ld, _p(s.pidx), N, OH, OW, Cp, PH, PW, st)
        if out is None:
            out = Act(self, self.empty(N, OH, OW, y_C, y_dt), y_C, y_C, y_C, y_dt) if y_C is not None else Act(self, self.empty(N, OH, OW, Cp, y_dt), s.Cout, s.gw_o, s.gwp_o, y_dt)
        s.out, s.ncopy = out, (y_C if y_C is not None else Cp)
        assert residual is None or (residual.Cp == Cp and residual.dt == self.dt)
        if sum_with is not None and (s.fuse_bias or residual is not None or y_dt != self.dt or s.ncopy != Cp or sum_with.dt != self.dt
                                     or (sum_with.N, sum_with.H, sum_with.W, sum_with.Cp) != (N, OH, OW, Cp) or out.ld % 8 or sum_with.ld % 8):
            raise RuntimeError("sum_with needs a plain same-dtype BN/activation output of the same geometry")
        if sum_with is not None:
            y2 = s.y2 = self._new_out(s)
            call.pn2_affine_act_sum(self.dt, _p(raw), raw_ld, out.ptr, out.ld, M, Cp, _p(s.scale), _p(s.shift), _relu_code(s.relu), sum_with.ptr, sum_with.ld, y2.ptr, y2.ld, st)
            if self.need_grad and sum_with.requires_grad:
                y2.galias = sum_with            # d(y + s)/ds = 1 and s has no other consumer: the sum's gradient lives in s's gradient storage
                y2.sum_of = (out, sum_with)
        elif s.pool:
            pass                      # (written above, pooled)
        elif not s.fuse_bias:
            # tee = (Act, c_lo): the output channels >= c_lo also go to that activation (Bottle2neck: spx[3] lands in the concat buffer, no copy launch)
            if tee is not None and residual is None and y_dt == self.dt and s.ncopy == Cp and core.TEE_CONCAT and tee[0].dt == self.dt and not (tee[1] % V or tee[0].ld % V or out.ld % V or raw_ld % V or Cp % V):
                call.pn2_affine_act_tee(self.dt, _p(raw), raw_ld, out.ptr, out.ld, M, Cp, _p(s.scale), _p(s.shift), _relu_code(s.relu), tee[0].ptr, tee[0].ld, tee[1], st)
                tee = None
            elif s.dual is not None:          # the residual is a BatchNorm output that was never written: both operands normalised here
                d = s.dual
                call.pn2_affine_act_dual(self.dt, _p(raw), raw_ld, _p(s.scale), _p(s.shift), _p(d.raw), d.raw_ld, _p(d.scale), _p(d.shift), out.ptr, out.ld, M, Cp, _relu_code(s.relu), st)
            else:
                call.pn2_affine_act(self.dt, _p(raw), raw_ld, y_dt, out.ptr, out.ld, M, s.ncopy, _p(s.scale), _p(s.shift),
                                    residual.ptr if residual is not None else C.c_void_p(0), residual.ld if residual is not None else 0, _relu_code(s.relu), st)
        if tee is not None:          # (a path without the second output: the slice is copied)
            call.pn2_copy(out.dt, _p(out.t[..., tee[1]:tee[1] + tee[0].Cp]), out.ld, tee[0].dt, tee[0].ptr, tee[0].ld, M, tee[0].Cp, 0, st)

    def _bwd_incoming(self, s):
        """s.dy: the gradient that arrived (after the sum_with share and the unfused pool backward); s.draw: where the gradient of raw goes; the ReLU mask: the stored output s.ymask, or from raw with s.msc / s.msh."""
        out, y2, sum_with, st, N, OH, OW, Cp, V, relu = s.out, s.y2, s.sum_with, s.st, s.N, s.OH, s.OW, s.Cp, s.V, s.relu
        if out.pool_prior is not None:
            self.flush_pool_prior(out)          # (no dgrad epilogue took the deferred pool backward of this output: apply it before the gradient is consumed)
        if y2 is not None and y2.grad_written and not y2.dual_done:          # the sum's gradient also flows into y (the other operand holds it already)
            if y2.galias is not None:
                assert not sum_with._written, "sum_with: the aliased operand received another gradient"
                sum_with.grad_written = True
            g2 = y2.grad_buf()
            go, oacc = out.grad_sink()
            call.pn2_copy(self.dt, _p(g2), g2.stride(2), self.dt, _p(go), go.stride(2), s.M, Cp, oacc, st)
            if y2.galias is None and sum_with.requires_grad:
                gs, sacc = sum_with.grad_sink()
                call.pn2_copy(self.dt, _p(g2), g2.stride(2), self.dt, _p(gs), gs.stride(2), s.M, Cp, sacc, st)
        dy = out.grad_buf()
        assert out.grad_written or out.child_written, "conv output never received a gradient"
        cvq = Cp // V
        s.quad = (s.pool and core.POOL_BWD_QUAD and OH % 2 == 0 and OW % 2 == 0 and cvq <= 256 and cvq & (cvq - 1) == 0 and dy.stride(2) % V == 0 and N * (OH // 2) * (OW // 2) < (1 << 24) - (1 << 21))
        if s.pool and not s.quad:          # the gradient of the (never stored) full-resolution BatchNorm output, as MaxPool2d's backward leaves it
            dyf = self.empty(N, OH, OW, Cp)
            call.pn2_maxpool3x3s2_bwd(self.dt, _p(dy), dy.stride(2), _p(s.pidx), _p(dyf), Cp, N, OH, OW, Cp, out.H, out.W, st)
            dy = dyf
        s.dy, s.dt_dy, s.Cdy = dy, out.dt, s.ncopy
        s.draw = s.draw_done if s.draw_done is not None else self.empty(N, OH, OW, Cp)
        s.ymask, s.msc, s.msh = (out if relu else None), None, None
        s.r6 = 1 if relu == 2 else 0          # relu: False / True (ReLU) / 2 (ReLU6: the mask also drops the saturated y == 6)
        if (s.bnb_ok or s.pool) and relu and s.residual is None and dy.stride(2) % V == 0:
            # ReLU mask recomputed from the raw conv output (fmaf(x, scale, shift) > 0, bit-identical to the forward):
            # the backward passes then do not read y at all
            s.ymask, s.msc, s.msh = None, s.scale, s.shift

    def _bn_sinks(self, bn):
        (gg, ga), (gb, gba) = self.pgrads.sink(bn.weight), self.pgrads.sink(bn.bias)
        assert ga == gba
        return gg, gb, ga

    def _bn_backward_quad(self, s, coef, sinks):
        # both BatchNorm passes form the incoming gradient per 2 x 2 input quad from the pooled gradient + argmax bytes: no pool-backward launch, no 176 x 176 gradient tensor
        dy, out, Cp, bn, st = s.dy, s.out, s.Cp, s.bn, s.st
        nb = 512          # workgroups = partial rows of the reduce (flat from 512 to 4096)
        p1, p2 = self.fbuf(nb, Cp), self.fbuf(nb, Cp)
        call.pn2_pool_bn_bwd_reduce(self.dt, _p(dy), dy.stride(2), _p(s.pidx), _p(s.raw), s.raw_ld, s.N, s.OH, s.OW, Cp, out.H, out.W, _p(s.mean), _p(s.invstd), _p(s.msc), _p(s.msh), _p(p1), _p(p2), nb, st)
        call.pn2_bn_bwd_finalize(_p(p1), _p(p2), nb, C.byref(s.bd), _p(bn.weight), _p(s.invstd), _p(sinks[0]), _p(sinks[1]), sinks[2], _p(coef), st)
        call.pn2_pool_bn_bwd_apply(self.dt, _p(dy), dy.stride(2), _p(s.pidx), _p(s.raw), s.raw_ld, s.N, s.OH, s.OW, Cp, out.H, out.W, _p(s.mean), _p(s.invstd), _p(coef), _p(s.msc), _p(s.msh), _p(s.draw), Cp, st)

    def _bn_backward_segs(self, s, segs, coef, sinks):
        # (part of) the statistics were left by dgrad epilogues; channel ranges nobody covered get a reduce pass of their own
        dy, raw, ymask, msc, st, nul = s.dy, s.raw, s.ymask, s.msc, s.st, C.c_void_p(0)
        sg = capi.BnSegs()
        sg.nseg = len(segs)
        for k_, (c0, nc, p1, p2, nb_, ldp) in enumerate(segs):
            if p1 is None:
                nb_ = call.pn2_bn_bwd_blocks(s.M, nc, self.dt)
                p1, p2, ldp = self.fbuf(nb_, nc), self.fbuf(nb_, nc), nc
                ym = ymask.t[..., c0:c0 + nc] if ymask is not None else None
                call.pn2_bn_bwd_reduce(self.dt, s.dt_dy, _p(dy[..., c0:c0 + nc]), dy.stride(2), nc, _p(ym), ym.stride(2) if ym is not None else 0, self.dt,
                                       _p(raw[..., c0:c0 + nc]), s.raw_ld, s.M, nc, _p(s.mean[c0:]), _p(s.invstd[c0:]), _p(p1), _p(p2), nb_,
                                       _p(msc[c0:]) if msc is not None else nul, _p(s.msh[c0:]) if msc is not None else nul, s.r6, st)
            sg.c0[k_], sg.nblk[k_], sg.ldp[k_], sg.p1[k_], sg.p2[k_] = c0, nb_, ldp, p1.data_ptr(), p2.data_ptr()
            self._keep.append((p1, p2))
        rg, racc = self._bwd_residual_sink(s)
        if self._bn_backward_dual(s, sg, coef, sinks, rg):
            return
        call.pn2_bn_bwd_finalize_seg(C.byref(sg), C.byref(s.bd), _p(s.bn.weight), _p(s.invstd), _p(sinks[0]), _p(sinks[1]), sinks[2], _p(coef), st)
        self._bn_bwd_apply(s, coef, s.draw, rg, racc)

    def _bn_backward_dual(self, s, sg, coef, sinks, rg):
        """BatchNorm + residual + ReLU whose residual is a BatchNorm output without activation (Bottle2neck's bn3 and downsample BatchNorm): when the dgrad epilogue that stored the
        masked gradient dz left the backward sums of BOTH (PN2_RES_STATS) and dz is the residual's gradient buffer, the two finalize launches go out as one table and one pass
        (pn2_bn_bwd_apply_dual) reads dz once for both raw gradients; the residual's producer record (Act.prod) then finds its own in draw_done.  -> whether it ran."""
        r, dy, V = s.residual, s.dy, s.V
        if not (core.DUAL_BNB_APPLY and r is not None and s.out.bnb is not None and s.out.bnb.res is r and s.out.grad_masked and rg is None and r.grad is dy
                and s.ymask is None and s.msc is None and s.dt_dy == self.dt and s.Cdy == s.Cp and dy.stride(2) % V == 0 and s.Cp % V == 0 and s.raw_ld % V == 0
                and r.prod is not None and r.prod.draw_done is None and (r.M, r.Cp, r.dt) == (s.M, s.Cp, self.dt) and r.prod.raw_ld % V == 0):
            return False
        rsegs = r.find_bstats()
        if len(rsegs) != 1 or rsegs[0][2] is None:
            return False
        st, d = s.st, r.prod
        _c0, _nc, q1, q2, nb_, ldp = rsegs[0]
        sg_r = capi.BnSegs()
        sg_r.nseg, sg_r.c0[0], sg_r.nblk[0], sg_r.ldp[0], sg_r.p1[0], sg_r.p2[0] = 1, 0, nb_, ldp, q1.data_ptr(), q2.data_ptr()
        self._keep.append((q1, q2))
        coef_r, sinks_r = self.fbuf(3 * r.Cp), self._bn_sinks(d.bn)
        self.lockstep("bnb.dual", [
            lambda: call.pn2_bn_bwd_finalize_seg(C.byref(sg), C.byref(s.bd), _p(s.bn.weight), _p(s.invstd), _p(sinks[0]), _p(sinks[1]), sinks[2], _p(coef), st),
            lambda: call.pn2_bn_bwd_finalize_seg(C.byref(sg_r), C.byref(d.bd), _p(d.bn.weight), _p(d.invstd), _p(sinks_r[0]), _p(sinks_r[1]), sinks_r[2], _p(coef_r), st)])
        draw_r = self.empty(r.N, r.H, r.W, r.Cp)
        call.pn2_bn_bwd_apply_dual(self.dt, _p(dy), dy.stride(2), s.M, s.Cp, _p(s.raw), s.raw_ld, _p(s.mean), _p(s.invstd), _p(coef), _p(s.draw), s.Cp,
                                   _p(d.raw), d.raw_ld, _p(d.mean), _p(d.invstd), _p(coef_r), _p(draw_r), r.Cp, st)
        d.draw_done = draw_r
        return True

    def _bn_backward_plain(self, b, mods, draw=None, coef=None, sinks=None, res_sink=None):
        """The plain BatchNorm backward of conv_bn_act, conv_bn_multi and EncoderOps.bn_after: one reduce pass over the operands b (st, dy, dt_dy, Cdy, ymask, raw, raw_ld, M, Cp, mean, invstd, msc, msh, r6), one finalize per
        BatchNorm of mods = [(bn, BnDesc, first column)], one apply pass -> the gradient of raw.  draw / coef / sinks: from callers that made them earlier (None: made here).  res_sink() -> (residual's gradient or None, accumulate)."""
        st, ym, nul = b.st, b.ymask, C.c_void_p(0)
        nb = call.pn2_bn_bwd_blocks(b.M, b.Cp, self.dt)
        p1, p2 = self.fbuf(nb, b.Cp), self.fbuf(nb, b.Cp)
        call.pn2_bn_bwd_reduce(self.dt, b.dt_dy, _p(b.dy), b.dy.stride(2), b.Cdy, ym.ptr if ym else nul, ym.ld if ym else 0, self.dt,
                               _p(b.raw), b.raw_ld, b.M, b.Cp, _p(b.mean), _p(b.invstd), _p(p1), _p(p2), nb, _p(b.msc), _p(b.msh), b.r6, st)
        coef = self.fbuf(3 * b.Cp) if coef is None else coef
        for bn, bd, off in mods:
            gg, gb, ga = sinks if sinks is not None else self._bn_sinks(bn)
            call.pn2_bn_bwd_finalize(_p(p1[:, off:]), _p(p2[:, off:]), nb, C.byref(bd), _p(bn.weight), _p(b.invstd[off:]), _p(gg), _p(gb), ga, _p(coef[off:]), st)
        rg, racc = res_sink() if res_sink is not None else (None, 0)
        draw = self.empty(*b.raw.shape[:3], b.Cp) if draw is None else draw
        self._bn_bwd_apply(b, coef, draw, rg, racc)
        return draw

    def _bn_bwd_apply(self, b, coef, draw, rg, racc):
        """draw = the gradient of raw from dy (masked by ymask or from raw) with the BatchNorm coefficient rows coef (None: no BatchNorm); rg: where the residual operand's gradient goes."""
        ym, nul = b.ymask, C.c_void_p(0)
        call.pn2_bn_bwd_apply(self.dt, b.dt_dy, _p(b.dy), b.dy.stride(2), b.Cdy, ym.ptr if ym else nul, ym.ld if ym else 0, self.dt, _p(b.raw), b.raw_ld, b.M, b.Cp, _p(b.mean), _p(b.invstd), _p(coef), _p(draw), b.Cp,
                              _p(rg), rg.stride(2) if rg is not None else 0, racc, _p(b.msc), _p(b.msh), b.r6, b.st)

    def _bwd_residual_sink(self, s):
        """-> (tensor, accumulate) where the apply pass leaves the residual operand's gradient (None: nowhere)."""
        residual, dy = s.residual, s.dy
        if s.out.grad_masked:
            s.ymask = None                  # dy already carries the ReLU mask (PN2_BNB_STORE_MASKED)
        if residual is not None and residual.requires_grad:
            if (s.out.grad_masked and residual.grad is None and residual.galias is None and residual.parent is None and not residual.grad_written
                    and tuple(dy.shape) == tuple(residual.t.shape) and dy.dtype == residual.t.dtype and dy.is_contiguous()):
                # d(out)/d(residual) = the ReLU mask: the masked dy IS the residual's gradient - share the buffer (it is dead here once dz
                # has been formed; later contributions to the residual's gradient accumulate into it in place)
                residual.grad = dy
                residual.grad_written = True
            else:
                return residual.grad_sink()
        return None, 0

    def _bwd_no_bn(self, s):
        """Backward of the output pass without a BatchNorm -> whether the bias gradient is done."""
        bias, dy = s.bias, s.dy
        if s.bn is not None:
            raise RuntimeError("backward through eval-mode BatchNorm is not supported")
        bias_done = bias is None
        if bias is not None and s.dt_dy == F32 and self.dt != F32 or (bias is not None and s.Cdy != s.Cp):
            gb, gba = self.pgrads.sink(bias)          # fp32 K-channel head maps: sum the fp32 gradient itself
            call.pn2_bias_grad(_p(dy), s.M, s.Cdy, _p(gb), gba, s.st)
            bias_done = True
        rg, racc = self._bwd_residual_sink(s)
        if s.ymask is None and rg is None and s.dt_dy == self.dt and s.Cdy == s.Cp and dy.stride(2) == s.Cp and dy.is_contiguous():
            s.draw = dy               # no BN, no activation, no residual (nn.Linear / biased conv): dz IS dy - no copy pass
        else:
            self._bn_bwd_apply(s, None, s.draw, rg, racc)
        return bias_done

    def _bwd_gate(self, s):
        # dz is the gradient of the GATED GEMM result: dzg = (1 - s) * dz feeds dgrad / wgrad, d gate[m] = -s * sum_c raw[m][c] * dz[m][c]
        gate, draw, M, Cp, st = s.gate, s.draw, s.M, s.Cp, s.st
        gc_, cacc = gate.grad_sink()
        dc = self.fbuf(M) if cacc else gc_
        dzg = draw if draw is not s.dy else self.alloc((s.N, s.OH, s.OW, Cp), self.tdt)
        call.pn2_ra_gate_post_bwd(self.dt, _p(s.raw), s.raw_ld, gate.ptr, _p(draw), Cp, _p(dzg), Cp, _p(dc), M, Cp, st)
        if cacc:
            call.pn2_copy(F32, _p(dc), 1, F32, _p(gc_), 1, M, 1, 1, st)
        s.draw = dzg

    def _wgrad(self, s, draw, Kp, weights, slab_key):
        """Weight gradients from draw, the [M][s.Cp] gradient of the (stacked) raw output: descriptor, tuner, splits, slab, launch + one reduce per weight, immediate or queued.  weights = [(weight, out_map, first row)]."""
        x, M, st = s.x, s.M, s.st
        wd, tco = _wgrad_desc(s.N, s.H, s.W, s.OH, s.OW, x.Cp, x.ld, s.Cp, s.k, Kp)
        nsplit = _wgrad_splits(M, wd, tco)
        rds = [self._pack_desc(w, s.x_map, o_map, False) for w, o_map, _off in weights]
        for rd in rds:
            rd.Rp = wd.Rp
        wd.tune, nsplit = self._tune_wgrad(wd, _p(draw), x.ptr, rds[0], nsplit, weights[0][0].shape)
        rq = self.grad_queue
        defer = rq is not None and rq.defer_wgrad
        if defer:
            nsplit = rq.table_splits(nsplit, M, x.Cp + s.Cp, wd, 4 if self.dt == F32 else 2)
        slab = self.fbuf(nsplit, wd.Rp, wd.Kp) if rq is None else rq.slab(slab_key, (nsplit, wd.Rp, wd.Kp), self.dev)
        # wgrad (+ slab reduce) only feeds the parameter gradient: with a gradient queue both are deferred into the table-driven launches of its flush
        if defer:
            rq.add_wgrad(self.mma, draw, x.ptr, x.t, slab, wd, nsplit, s.flops)
        else:
            capi.WORK.update(flops=s.flops, tag="", shape=s.shape)
            call.pn2_conv_wgrad(self.mma, _p(draw), x.ptr, _p(slab), C.byref(wd), nsplit, st)
        for (w, _o_map, off), rd in zip(weights, rds):
            gwt, gwa = self.pgrads.sink(w)
            if rq is None:
                call.pn2_wgrad_reduce(_p(slab[:, off:]), _p(gwt), C.byref(rd), nsplit, gwa, st)
            else:
                rq.add_reduce(slab[:, off:], gwt, rd, nsplit, gwa)

    def _dgrad_patch(self, s):
        # patchify conv (kernel == stride): every input pixel sees exactly one tap -> GEMM over the patches + depth-to-space
        x, draw, N, OH, OW, KH, KW, Cp, st = s.x, s.draw, s.N, s.OH, s.OW, s.KH, s.KW, s.Cp, s.st
        gx, gxa = x.grad_sink()
        Ct = KH * KW * x.Cp
        Rp2, Kp2 = rup(Ct, 128), rup(Cp, 128)
        wp2 = self.alloc((Rp2, Kp2), self.tdt)
        call.pn2_pack_patch_weight(self.dt, _p(s.w), _p(wp2), s.Cout, s.Cin, KH, KW, x.Cp, Rp2, Kp2, st)
        tpatch = self.empty(N, OH, OW, Ct)
        dd = _conv_desc(N, OH, OW, OH, OW, Cp, Cp, Ct, Ct, Kp=Kp2)
        dd.flags |= self._tune_gemm(dd, _p(draw), wp2, s.M, Ct) << 8
        capi.WORK.update(flops=s.flops, tag=":dgrad", shape=s.shape + " patch")
        call.pn2_conv_gemm(self.mma, _p(draw), _p(wp2), _p(tpatch), C.c_void_p(0), C.c_void_p(0), C.byref(dd), st)
        call.pn2_depth_to_space(self.dt, _p(tpatch), Ct, _p(gx), gx.stride(2), N, s.H, s.W, OH, OW, KH, x.Cp, gxa, st)

    def _dgrad_small_cin(self, s):
        # few-channel strided conv (EMCADNet's patch embedding behind the 1 -> 3 stem): only the taps that land on an output pixel
        gx, gxa = s.x.grad_sink()
        capi.WORK.update(flops=s.flops, tag=":dgrad", shape=s.shape + " small-cin")
        call.pn2_conv_dgrad_small_cin(self.dt, _p(s.draw), s.Cp, _p(s.w), _p(gx), gx.stride(2), s.N, s.H, s.W, s.OH, s.OW, s.Cout, s.Cin, s.KH, s.KW, s.sh, s.ph, gxa, s.st)

    def _ep_describe(self, x, dual):          # description-only ConvEp of the dgrad that completes x's gradient (dual: of both operands of the sum x is): what the tuner needs to know
        ep = capi.ConvEp()
        for t_, a_ in ((ep.a, x.sum_of[0] if dual else x), (ep.b, x.sum_of[1] if dual else None)):
            if a_ is not None and a_.bnb is not None:
                self._fill_bnb(t_, a_, 0)
        if dual:
            ep.b.out = 1
        return ep

    def _dgrad_gemm(self, s):
        """The data gradient as a GEMM with the transposed weight panel: plain, global split-K + reduce, or with a BatchNorm-backward epilogue (_dgrad_ep)."""
        x, draw, N, H, W, KH, KW, Cp, V, st = s.x, s.draw, s.N, s.H, s.W, s.KH, s.KW, s.Cp, s.V, s.st
        wt, ptd = self.pack(s.w, s.x_map, s.o_map, True)
        # a deferred AvgPool2d(2, 2) backward on x (SpatialOps.avgpool(fold_bwd=True)): this dgrad completes x's gradient with a BatchNorm-backward epilogue and
        # nothing has been written to it yet -> the epilogue adds 1/4 of the pooled gradient itself (pn2_conv_ep.pool); anything else: the plain pool-backward launch
        pool_ok = (x.pool_prior is not None and core.BNB_EPILOGUE and s.x_last and not x.grad_written and x.bnb is not None and x.sum_of is None and x.Cp % V == 0 and x.pool_prior[0].shape[3] == x.Cp and self.dt == x.dt and x.grad_buf().stride(2) % V == 0
                   and self._ksplit(N * H * W, KH * KW * Cp, x.Cp) == 1)
        if x.pool_prior is not None and not pool_ok:
            self.flush_pool_prior(x)
        (gx, gxa), Mx = x.grad_sink(), N * H * W
        dd = _conv_desc(N, s.OH, s.OW, H, W, Cp, Cp, x.Cp, gx.stride(2), s.k, 1, ptd.Kp, capi.CONV_ACCUM if gxa else 0)
        ks = self._ksplit(Mx, KH * KW * Cp, x.Cp) if gx.stride(2) == x.Cp else 1
        dual = x.sum_of is not None and x.galias is x.sum_of[1] and x.sum_of[0].requires_grad
        want_ep = bool(core.BNB_EPILOGUE and s.x_last and x.Cp % V == 0 and gx.stride(2) % V == 0 and (x.bnb is not None or dual))
        if ks > 1:
            # as in the forward: intra-workgroup split-K instead of partial tiles + reduce.  The probe asks the tuner with THE KEY THE LAUNCH WILL USE (a launch
            # with a BatchNorm-backward epilogue is tuned with it: other LDS budget, other key); if that code is not of the split-K class (no tile of it fits
            # next to the epilogue's operand tiles, or no tuner) the global split-K + reduce pair stays - never a long-K launch with neither
            probe = self._ep_describe(x, dual) if want_ep else None
            if want_ep and dual and x.sum_of[0].grad_written:
                dd.flags |= capi.CONV_ACCUM
            if self._tune_gemm(dd, _p(draw), wt, Mx, x.Cp, probe) & 0xC0:
                ks = 1
            dd.flags = capi.CONV_ACCUM if gxa else 0
        capi.WORK.update(flops=s.flops, tag=":dgrad", shape=s.shape)
        if ks > 1:
            ws = self.fbuf(ks, Mx, x.Cp)
            dd.flags = ((2 | (1 << 2) | ((3 if x.Cp > 64 else 2) << 4)) << 8) | (ks << 16)
            call.pn2_conv_gemm(self.mma, _p(draw), _p(wt), _p(gx), _p(ws), C.c_void_p(0), C.byref(dd), st)
            call.pn2_conv_splitk_reduce(self.dt, _p(ws), ks, Mx, x.Cp, _p(gx), x.Cp, C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), gxa, st)
        elif want_ep:
            self._dgrad_ep(s, dd, wt, gx, gxa, dual, pool_ok)
        else:
            dd.flags |= self._tune_gemm(dd, _p(draw), wt, Mx, x.Cp) << 8
            call.pn2_conv_gemm(self.mma, _p(draw), _p(wt), _p(gx), C.c_void_p(0), C.c_void_p(0), C.byref(dd), st)

    def _dgrad_ep(self, s, dd, wt, gx, gxa, dual, pool_ok):
        """The dgrad GEMM whose epilogue takes the BatchNorm-backward statistics of the gradient it completes (x's, or those of both operands of the sum x is)."""
        x, draw, V, st, Mx = s.x, s.draw, s.V, s.st, s.N * s.H * s.W
        ep = self._ep_describe(x, dual)
        if dual and x.sum_of[0].grad_written:
            dd.flags |= capi.CONV_ACCUM
        if pool_ok:
            assert not gxa and not dual
            dd.flags |= capi.CONV_ACCUM
            ep.pool, ep.ld_pool = x.pool_prior[0].data_ptr(), x.pool_prior[0].stride(2)
        tcode = self._tune_gemm(dd, _p(draw), wt, Mx, x.Cp, ep)
        dd.flags |= tcode << 8
        nbx = self._stat_blocks(Mx, x.Cp, tcode)
        ep = capi.ConvEp()
        if pool_ok:
            ep.pool, ep.ld_pool = x.pool_prior[0].data_ptr(), x.pool_prior[0].stride(2)
        if dual:
            # x = u + v (Bottle2neck's sp + spx[i]): the gradient goes to BOTH operands - accumulated into u's (the concat buffer slice
            # conv3's dgrad wrote), stored as v's (aliased by x) - each with the statistics of its own BatchNorm
            u, v = x.sum_of
            gu, gua = u.grad_sink()
            assert gu.stride(2) % V == 0
            dd.ld_out, dd.flags = gu.stride(2), (dd.flags & ~capi.CONV_ACCUM) | (capi.CONV_ACCUM if gua else 0)
            self._fill_bnb(ep.a, u, nbx)
            ep.b.out, ep.b.ld_out = gx.data_ptr(), gx.stride(2)
            self._fill_bnb(ep.b, v, nbx)
            v.grad_written = True
            x.dual_done = True
            u._sealed = v._sealed = True
            call.pn2_conv_gemm_ep(self.mma, _p(draw), _p(wt), _p(gu), C.byref(dd), C.byref(ep), st)
        else:
            self._fill_bnb(ep.a, x, nbx, ep, tcode)
            call.pn2_conv_gemm_ep(self.mma, _p(draw), _p(wt), _p(gx), C.byref(dd), C.byref(ep), st)
        if pool_ok and x.pool_prior is not None:
            x.pool_prior = None
            self._pending_pool.remove(x)
        x._sealed = True

    def _padded_bias(self, bias, Cout, Cout_p):
        """[Cout_p] fp32 row: the bias in its first Cout slots, zeros behind.  With a persistent pack cache the row persists (its pad slots are written once) and a step
        refreshes it with ONE copy instead of a fill + a copy (the K-channel head convs of pranet.py:104-105,303-325: 4 launches per step fewer)."""
        if Cout_p == Cout:
            return bias.detach()
        cache = self.pack_cache
        if cache is None:
            row = torch.zeros(Cout_p, dtype=torch.float32, device=self.dev)
        else:
            rows = cache.__dict__.setdefault("bias_rows", {})
            row = rows.get((id(bias), Cout_p))
            if row is None:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("run an eager step before capturing (the padded bias rows are created then)")
                row = rows[(id(bias), Cout_p)] = torch.zeros(Cout_p, dtype=torch.float32, device=self.dev)
                cache.__dict__.setdefault("bias_keep", []).append(bias)          # (id(bias) stays unique while the row exists)
        row[:Cout].copy_(bias.detach())
        return row

    def _bn_eval_rows(self, bn, M, Cout_p, Cout, gw_o, gwp_o, bias=None):
        """-> (scale, shift) fp32 [Cout_p] rows of an eval-mode BatchNorm (bias of the conv in front folded into shift).  With a BnFoldCache the rows persist and
        were refreshed at the start of this forward; a layer seen for the first time is folded here and joins the cache."""
        bd = _bn_desc(bn, M, Cout_p, Cout, gw_o, gwp_o)
        fold = self.bn_fold if bias is None else None
        key = (id(bn), Cout_p, gw_o, gwp_o)
        if fold is not None and key in fold.entries:
            par = fold.entries[key]
            return par[0], par[1]
        par = torch.empty((2, Cout_p), dtype=torch.float32, device=self.dev) if fold is not None else self.fbuf(2, Cout_p)
        call.pn2_bn_eval_prepare(C.byref(bd), _p(bn.weight), _p(bn.bias), _p(bn.running_mean), _p(bn.running_var), _p(par[0]), _p(par[1]), _stream())
        if bias is not None:
            par[1][:Cout] += bias.detach() * par[0][:Cout]
        if fold is not None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("run an eager forward before capturing (the BatchNorm fold table is built then)")
            fold.add(key, bn, par, bd)
        return par[0], par[1]

    def _tile_m(self, M, Cout, tune):
        bm = (tune >> 2) & 3
        return (64 if bm == 1 else 128) if bm else call.pn2_conv_tile_m(M, Cout, self.mma)

    def _fill_bnb(self, t, act, nblk, ep=None, tcode=0):
        """Describe `act`'s BatchNorm to a dgrad epilogue target and register the partial rows it will leave."""
        b = act.bnb
        if b is None:
            t.mode = 0
            return
        t.mode = capi.BNB_STATS | (capi.BNB_MASK_Y if b.ymask is not None else (capi.BNB_MASK_RAW if b.relu else 0))
        if b.ymask is not None and core.MASKED_STORE and nblk and b.split == 0 and act.parent is None:
            # BN + residual + ReLU: the masked gradient is also the residual branch's gradient - store it masked, the producer aliases it
            t.mode |= capi.BNB_STORE_MASKED
            act.grad_masked = True
        t.raw, t.ld_raw = b.raw.data_ptr(), b.raw.stride(2)
        if b.ymask is not None:
            t.y, t.ld_y = b.ymask.data_ptr(), b.ymask.stride(2)
        t.par, t.ps = b.par.data_ptr(), b.par.stride(0)
        Cp = act.Cp
        if b.split:
            t.split = b.split
            if b.par2 is not None:
                t.raw2, t.par2 = b.raw2.data_ptr(), b.par2.data_ptr()
        if nblk == 0:               # description only (the tuner supplies its own partial rows)
            return
        p1, p2 = self.fbuf(nblk, Cp), self.fbuf(nblk, Cp)
        t.p1, t.p2, t.ldp = p1.data_ptr(), p2.data_ptr(), Cp
        bm_, bn_ = (tcode >> 2) & 3, (tcode >> 4) & 3
        if (ep is not None and core.RES_STATS and b.res is not None and (t.mode & capi.BNB_STORE_MASKED) and self.dt == BF16 and bm_ and bn_
                and (64 << (bm_ - 1)) * (16 << bn_) <= 4096 and not b.res.grad_written and b.res.galias is None and b.res.grad is None):
            # the residual operand is a BatchNorm output without activation whose gradient will BE the masked dz stored here: its backward sums ride in this
            # epilogue too (LDS-DMA / matrix-core form: tiles of <= 4096 elements); its producer then finds them like any other epilogue statistics
            rb = b.res.bnb
            c = ep.c
            c.mode, c.raw, c.ld_raw, c.par, c.ps = capi.BNB_STATS, rb.raw.data_ptr(), rb.raw.stride(2), rb.par.data_ptr(), rb.par.stride(0)
            q1, q2 = self.fbuf(nblk, Cp), self.fbuf(nblk, Cp)
            c.p1, c.p2, c.ldp = q1.data_ptr(), q2.data_ptr(), Cp
            b.res.add_bstats(0, Cp, q1, q2, nblk, Cp)
        if b.split:
            t.split = b.split
            if b.par2 is not None:
                assert b.raw2.stride(2) == b.raw.stride(2) and b.par2.stride(0) == b.par.stride(0)
                t.raw2, t.par2 = b.raw2.data_ptr(), b.par2.data_ptr()
                b.tail.add_bstats(0, Cp - b.split, p1[:, b.split:], p2[:, b.split:], nblk, Cp)
            act.add_bstats(0, b.split, p1, p2, nblk, Cp)
        else:
            act.add_bstats(0, Cp, p1, p2, nblk, Cp)

    def concat_bnb(self, cat, raw, par, split=0, tail=None):
        """Declare that the channels [0, split or all) of the concat buffer `cat` were written by train-mode conv+BN(+ReLU) ops whose raw outputs /
        parameter rows sit in the matching channel slices of `raw` / `par` (conv_bn_act(raw_out=, par_out=)); channels >= split are a copy of the
        BN+ReLU output `tail` (None: they carry no BatchNorm).  The dgrad that completes cat's gradient can then take all those BatchNorms'
        backward statistics in one epilogue."""
        if not (core.BNB_EPILOGUE and self.need_grad and self.training):
            return
        tb = tail.bnb if tail is not None else None
        if tail is not None and (tb is None or not tb.relu or tb.ymask is not None):
            return
        r2 = p2 = None
        if tb is not None:
            # raw2 / par2 are indexed with cat's local column: shift the tail's views back by `split` columns
            tr, off = tail.root()
            rb = tr.bnb
            if rb is None or off != split or rb.raw.stride(2) != raw.stride(2) or rb.par.stride(0) != par.stride(0):
                return
            r2, p2 = rb.raw, rb.par
        cat.bnb = Bnb(raw, par, True, None, split, r2, p2, tail)

    # ------------------------------------------------------------------ fused 1x1 reducers sharing one input
    def conv_bn_multi(self, x, mods):
        """[BN_j(conv_j(x)) for j] for bias-free 1x1 / stride-1 BasicConv2d-style modules `mods` (each has .conv, .bn; no ReLU).

        The RFB branches, conv_res and the RA stage's conv1 all read the same encoder map (pranet.py:52,55,61,67,73,303,312,320):
        their weights are packed side by side into ONE panel so the map is read once in forward, dx is written once in dgrad
        (instead of J read-modify-write passes) and wgrad reads it once.  BatchNorm stays per module (own gamma/beta/running stats).
        Returns the channel-slice views of the fused [M][sum Cout] output."""
        convs = [m.conv for m in mods]
        for c in convs:
            assert c.kernel_size == (1, 1) and c.stride == (1, 1) and c.padding == (0, 0) and c.bias is None and c.in_channels == x.C
        couts = [c.out_channels for c in convs]
        assert all(co % 8 == 0 for co in couts)
        offs = [sum(couts[:j]) for j in range(len(couts))]
        Ct = sum(couts)
        N, H, W = x.N, x.H, x.W
        M = N * H * W
        train = self.training
        # the same kind of record as conv_bn_act's: one 1x1 conv with the stacked output width Ct
        s = SimpleNamespace(x=x, mods=mods, convs=convs, couts=couts, offs=offs, N=N, H=H, W=W, OH=H, OW=W, M=M, Cp=Ct, k=(1, 1, 1, 0, 0, 1, 1), x_map=(x.gw, x.gwp, x.Cp),
                            Kp=rup(x.Cp, 128), st=_stream(), train=train, flops=2 * M * Ct * x.C, shape=f"{x.C}->{'+'.join(map(str, couts))} k1x1 s1 d1 {N}x{H}x{W}")
        wp = self._multi_panel(s, False)
        cd = _conv_desc(N, H, W, H, W, x.Cp, x.ld, Ct, Ct, Kp=s.Kp, flags=capi.CONV_STATS if train else 0)
        tune = self._tune_gemm(cd, x.ptr, wp, M, Ct)
        cd.flags |= tune << 8
        psum, psq, nblk, tile_rows = None, None, 0, 0
        if train:
            nblk = self._stat_blocks(M, Ct, tune)
            tile_rows = self._tile_m(M, Ct, tune)
            psum, psq = self.fbuf(nblk, Ct), self.fbuf(nblk, Ct)
        capi.WORK.update(flops=s.flops, tag=":fwd", shape=s.shape)
        if core.EVAL_FUSE and not train and not self.need_grad:
            return self._multi_eval_fused(s, cd, tune, wp)
        s.raw, s.raw_ld = self.empty(N, H, W, Ct), Ct
        call.pn2_conv_gemm(self.mma, x.ptr, _p(wp), _p(s.raw), _p(psum), _p(psq), C.byref(cd), s.st)
        scale, shift = self.fbuf(Ct), self.fbuf(Ct)
        s.mean, s.invstd = (self.fbuf(Ct), self.fbuf(Ct)) if train else (None, None)
        s.bds = []
        for m, co, off in zip(mods, couts, offs):
            s.bds.append(_bn_desc(m.bn, M, co, co, co, co, Ct, tile_rows))
            rows = [r[off:] if r is not None else None for r in (scale, shift, s.mean, s.invstd)]
            self._bn_forward(m.bn, s.bds[-1], rows, psum[:, off:] if train else None, psq[:, off:] if train else None, nblk)
        out = s.out = Act(self, self.empty(N, H, W, Ct), Ct, Ct, Ct, self.dt)
        call.pn2_affine_act(self.dt, _p(s.raw), Ct, self.dt, out.ptr, out.ld, M, Ct, _p(scale), _p(shift), C.c_void_p(0), 0, 0, s.st)
        if self.need_grad:
            self.record(partial(self._multi_bwd, s))
        return [out.slice(off, off + co) for co, off in zip(couts, offs)]

    def _multi_panel(self, s, transposed):
        """The modules' weights side by side in one packed panel (transposed: the dgrad's)."""
        convs, x_map, Ct = s.convs, s.x_map, s.Cp
        Rp, Kp = rup(Ct, 128), s.Kp
        Rt, Kt = rup(s.x.Cp, 128), rup(Ct, 128)          # transposed (dgrad) panel
        cache = self.pack_cache
        key = ("multi", tuple(id(c.weight) for c in convs), transposed, x_map, self.dt)
        if cache is not None and key in cache.entries:
            return cache.entries[key][0]
        wp = torch.zeros((Rt, Kt) if transposed else (Rp, Kp), dtype=self.tdt, device=self.dev)
        for c, co, off in zip(convs, s.couts, s.offs):
            d = self._pack_desc(c.weight, x_map, (co, co, co), transposed)
            if transposed:
                d.Rp, d.Kp, d.ld, d.koff = Rt, co, Kt, off          # columns [off, off+co) of every row
                dst = wp
            else:
                d.Rp, d.Kp = co, Kp                                  # rows [off, off+co)
                dst = wp[off:]
            call.pn2_pack_weight(self.dt, _p(c.weight), _p(dst), C.byref(d), s.st)
            if cache is not None:
                cache.add(key + (off,), c.weight, dst, d)
        if cache is not None:
            cache.entries[key] = (wp, None)
        return wp

    def _multi_eval_fused(self, s, cd, tune, wp):
        # eval mode: the folded BatchNorms of all the reducers ride in the GEMM epilogue (pn2_conv_gemm_affine) - no raw output, no normalise pass
        mods, Ct, M, st = s.mods, s.Cp, s.M, s.st
        fold = self.bn_fold
        key = ("multi",) + tuple(id(m.bn) for m in mods)
        par = fold.entries.get(key) if fold is not None else None
        if par is None:
            par = torch.empty((2, Ct), dtype=torch.float32, device=self.dev) if fold is not None else self.fbuf(2, Ct)
            for m, co, off in zip(mods, s.couts, s.offs):
                bn = m.bn
                bd = _bn_desc(bn, M, co, co, co, co)
                call.pn2_bn_eval_prepare(C.byref(bd), _p(bn.weight), _p(bn.bias), _p(bn.running_mean), _p(bn.running_var), _p(par[0][off:]), _p(par[1][off:]), st)
                if fold is not None:
                    if torch.cuda.is_current_stream_capturing():
                        raise RuntimeError("run an eager forward before capturing (the BatchNorm fold table is built then)")
                    fold.add(key, bn, par, bd, off)
        out = Act(self, self.empty(s.N, s.H, s.W, Ct), Ct, Ct, Ct, self.dt)
        cd.flags = (tune << 8) | capi.CONV_AFFINE
        call.pn2_conv_gemm_affine(self.mma, s.x.ptr, _p(wp), out.ptr, _p(par[0]), _p(par[1]), C.c_void_p(0), 0, C.byref(cd), st)
        return [out.slice(off, off + co) for co, off in zip(s.couts, s.offs)]

    def _multi_bwd(self, s):
        x, out, Ct, N, H, W = s.x, s.out, s.Cp, s.N, s.H, s.W
        st = s.st = _stream()
        if not s.train:
            raise RuntimeError("backward through eval-mode BatchNorm is not supported")
        dy = out.grad_buf()
        assert out.grad_written or out.child_written
        s.dy, s.dt_dy, s.Cdy, s.ymask, s.msc, s.msh, s.r6 = dy, self.dt, Ct, None, None, None, 0
        draw = self._bn_backward_plain(s, [(m.bn, bd, off) for m, bd, off in zip(s.mods, s.bds, s.offs)])
        self._wgrad(s, draw, s.Kp, [(c.weight, (co, co, co), off) for c, co, off in zip(s.convs, s.couts, s.offs)], tuple(id(c.weight) for c in s.convs))
        if x.requires_grad:
            wt = self._multi_panel(s, True)
            gx, gxa = x.grad_sink()
            dd = _conv_desc(N, H, W, H, W, Ct, Ct, x.Cp, gx.stride(2), transposed=1, Kp=rup(Ct, 128), flags=capi.CONV_ACCUM if gxa else 0)
            dd.flags |= self._tune_gemm(dd, _p(draw), wt, s.M, x.Cp) << 8
            capi.WORK.update(flops=s.flops, tag=":dgrad", shape=s.shape)
            call.pn2_conv_gemm(self.mma, _p(draw), _p(wt), _p(gx), C.c_void_p(0), C.c_void_p(0), C.byref(dd), st)

    # ------------------------------------------------------------------ PVTv2 encoder ops (lib/pvtv2.py)
    def colsum_finalize(self, part, nblk, Cc, ld, out, accumulate):
        """out[:Cc] (+)= sum of the nblk partial rows.  These sums only feed parameter gradients: they are queued and run as ONE
        table-driven launch per flush (end of backward / before a gradient bucket leaves), not one launch each."""
        if not core.DEFER_COLSUM or self.grad_queue is None:      # (without a persistent queue the job table would be rebuilt and uploaded every step)
            call.pn2_colsum_finalize(_p(part), nblk, Cc, ld, _p(out), accumulate, _stream())
            return
        if accumulate:                  # a second contribution to the same gradient must see the first one finished
            self.flush_colsum()
        self.cjobs.append((part.data_ptr(), out.data_ptr(), nblk, Cc, ld, accumulate))
        self.ckeep.append((part, out))  # the partial rows must not be recycled before the launch is queued

    def flush_colsum(self):
        """Run the queued column sums (one pn2_colsum_multi per dtype) and then their finalisations (one pn2_colsum_finalize_multi)."""
        if not self.cjobs and not self.cin:
            return
        sig = (tuple(self.cin), tuple(self.cjobs))
        cache = self.grad_queue.ccache if self.grad_queue is not None else None
        hit = cache.get(self.cseg) if cache is not None else None
        if hit is None or hit[0] != sig:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("run two eager steps before capturing (the deferred-launch tables are built then)")
            launches = []
            for dt in sorted({j[0] for j in self.cin}):
                arr, blocks = [], []
                for d_, ptr, part, ld, M, Cc in self.cin:
                    if d_ != dt:
                        continue
                    j = capi.ColsumInJob()
                    j.dy, j.partial, j.ld, j.M, j.C = ptr, part, ld, M, Cc
                    nb = call.pn2_colsum_job_blocks(dt, C.byref(j))
                    if nb < 1:
                        raise RuntimeError("unsupported column-sum geometry")
                    arr.append(j); blocks.append(nb)
                launches.append(("s", dt, len(arr)) + _job_table(capi.ColsumInJob, arr, blocks))
            if self.cjobs:
                arr = []
                for part, out, nblk, Cc, ld, acc in self.cjobs:
                    j = capi.ColsumJob()
                    j.partial, j.out, j.nblk, j.C, j.ld, j.accumulate = part, out, nblk, Cc, ld, acc
                    arr.append(j)
                launches.append(("f", 0, len(arr)) + _job_table(capi.ColsumJob, arr, [call.pn2_colsum_finalize_blocks(j.C) for j in arr]))
            hit = (sig, launches)
            if cache is not None:
                cache[self.cseg] = hit
        st = _stream()
        for kind, dt, n, table, bstart, nblocks in hit[1]:
            if kind == "s":
                call.pn2_colsum_multi(dt, _p(table), _p(bstart), n, nblocks, st)
            else:
                call.pn2_colsum_finalize_multi(_p(table), _p(bstart), n, nblocks, st)
        self.ctables.append(hit)        # the tables must outlive the launches
        self.cseg += 1
        self.cjobs, self.cin, self.ckeep = [], [], []

    def colsum(self, t, M, Cp, Cc, out, accumulate):
        """out[:Cc] (+)= column sums of the [M][Cp] tensor t (bias gradients).  With a gradient queue both passes are deferred into the
        table-driven launches of flush_colsum (t stays alive in the step arena)."""
        st = _stream()
        dt = F32 if t.dtype == torch.float32 else BF16
        nb = call.pn2_rows_blocks(M, call.pn2_colsum_unit(dt, Cp))
        part = self.fbuf(nb, Cp)
        if core.DEFER_COLSUM and self.grad_queue is not None:
            self.cin.append((dt, t.data_ptr(), part.data_ptr(), Cp, M, Cp))
            self.ckeep.append(t)
        else:
            call.pn2_colsum(dt, _p(t), Cp, M, Cp, _p(part), nb, st)
        self.colsum_finalize(part, nb, Cc, Cp, out, accumulate)

    def linear(self, x, lin, residual=None):
        """nn.Linear (+ residual add) over the channels of NHWC tokens."""
        return self.conv_bn_act(x, _LinearAsConv(lin), None, bias=lin.bias, residual=residual)

    def conv_bias(self, x, conv):
        """biased nn.Conv2d without BN (patch embedding pvtv2.py:167, spatial reduction :70)."""
        return self.conv_bn_act(x, conv, None, bias=conv.bias)

