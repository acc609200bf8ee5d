"""One launch of every template rung that the host launch ladders of pn2_tail.hip, pn2_eval.hip, pn2_input.hip and pn2_seg.hip select and that no other GPU test
reaches.  The rungs and the tests that launch them:

    tail_fwd_k<P>, tail_one_k<P>          P = 4: test_gpu_parity.py::test_dsra_tail_band_kernels_vs_oracle_and_row_kernels;  P = 1, 2, 3: HERE
    seg_labels_k<mode>                    mode 0, 1, 2: test_gpu_seg_labels_up.py::test_fused_labels_exact_on_dyadic_maps (its unfused path, voleval.predict_labels)
    seg_labels_up_k<mode, KV, vec>        every mode with KV = 1, 3 (vec on and off) and KV = 1, 4 (vec on): the same test (K = 2, 9 at ld = K; K = 4, 16 and ld = 16);
                                          KV = 2 (vec on and off) and KV = 4 with vec off: HERE (K = 5 and 13)
    tail_minmax_batch_k / tail_bytes_batch_k<4>, <1>     test_gpu_eval_batch.py::test_tail_batch_bit_for_bit[sum4] and [last]
    input_batch_height_k<true>, <false>   test_gpu_input_batch.py::test_batch_entries_bit_for_bit[32-16] / [32-1] and [30-16]

Every case calls the entry point at the C ABI and is held to the reference and the tolerances of the neighbouring rung's test."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seglabelupref as R

pytestmark = pytest.mark.gpu
dev = "cuda"


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()
    yield


def relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def rell2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


# N, S: 64 keeps magnifications 8 and 16 (the one-pass kernel's geometry); 100 leaves a 4-row last band and is served by the row kernels alone
@pytest.mark.parametrize("N,S", [(2, 64), (1, 100)])
@pytest.mark.parametrize("P", [1, 2, 3])
def test_dsra_tail_row_and_one_pass_kernels_with_fewer_than_four_pairs(P, N, S, monkeypatch):
    """pn2_dsra_tail_fwd / _bwd on the row kernels (PN2_TAIL_BAND=0: tail_fwd_k<P>) and pn2_dsra_tail_fwd_bwd (tail_one_k<P>, without the image-sum accumulators:
    loss_total_k closes it) for P = 1, 2, 3 pairs, against the oracle's structure_loss on F.interpolate'd maps in float64 with autograd for the low-res
    gradients: relmax < 2e-6 on the maps, 5e-6 relative on the losses, relmax < 2e-4 and rell2 < 2e-5 on the gradients."""
    from pn2 import capi
    from pn2.capi import call
    from oracle import pranet_oracle as O
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(1000 + 10 * S + P)
    sizes = [S // 8, S // 16, S // 8][:P]
    src_cpu = [(torch.randn(N, h, h, generator=g) * 2) for h in sizes + sizes]
    mask_cpu = (torch.rand(N, 1, S, S, generator=g) < 0.3).float()
    mask_cpu[:, :, S // 4: S // 2, S // 3: 2 * S // 3] = 1.0
    leaves = [t.double().requires_grad_(True) for t in src_cpu]
    ups = [F.interpolate(t[:, None], size=(S, S), mode="bilinear", align_corners=False) for t in leaves]
    ref_losses = [O.structure_loss(ups[j], ups[P + j], mask_cpu.double(), 1 - mask_cpu.double()) for j in range(P)]
    sum(ref_losses).backward()
    ref_grads = [t.grad.float() for t in leaves]
    ups32 = [F.interpolate(t[:, None], size=(S, S), mode="bilinear", align_corners=False).reshape(N, S, S) for t in src_cpu]
    one_pass = S == 64
    for band in (("F", "0") if one_pass else ("0",)):          # (S = 100 has no one-pass geometry: the row kernels alone)
        monkeypatch.setenv("PN2_TAIL_BAND", "2" if band == "F" else band)
        srcs = [t.to(dev) for t in src_cpu]
        base = [torch.randn_like(t) * float(ref_grads[j].abs().max()) for j, t in enumerate(srcs)]          # the gradient already in the sinks that accumulate
        dsrcs = [base[j].clone() if j % 3 == 0 else torch.empty_like(t) for j, t in enumerate(srcs)]
        mask = mask_cpu.reshape(N, S, S).to(dev).contiguous()
        weit = torch.empty_like(mask)
        call.pn2_loss_weights(ptr(mask), ptr(weit), N, S, S, 31, st)
        d = capi.TailDesc()
        d.N, d.OH, d.OW, d.P, d.align_corners = N, S, S, P, 0
        for j, (s_, ds) in enumerate(zip(srcs, dsrcs)):
            m, h = d.maps[j], s_.shape[1]
            m.src, m.dsrc, m.h, m.w, m.rh, m.rw, m.accumulate = s_.data_ptr(), ds.data_ptr(), h, h, h / S, h / S, (1 if j % 3 == 0 else 0)
        nb = call.pn2_dsra_tail_blocks(S)
        lat = torch.empty(2 * P, N, S, S, device=dev)
        partial = torch.empty(P, N, nb, 5, device=dev)
        sums, wsum, loss = torch.empty(P, N, 4, device=dev), torch.empty(N, device=dev), torch.empty(P + 1, device=dev)
        fused = int(call.pn2_dsra_tail_fused_ok(C.byref(d)))
        assert fused == (1 if band == "F" and one_pass else 0), (band, fused)
        if band == "F":
            need = int(call.pn2_dsra_tail_fused_scratch(C.byref(d)))
            scratch, per = torch.empty(need, device=dev), torch.empty(P, N, device=dev)
            call.pn2_dsra_tail_fwd_bwd(C.byref(d), ptr(lat), ptr(mask), ptr(weit), ptr(partial), ptr(sums), ptr(wsum), ptr(per), ptr(loss), 1.0, ptr(scratch), need, None, st)
        else:
            assert int(call.pn2_dsra_tail_scratch(C.byref(d))) == 0
            call.pn2_dsra_tail_fwd(C.byref(d), ptr(lat), ptr(mask), ptr(weit), ptr(partial), ptr(sums), ptr(wsum), ptr(loss), st)
            call.pn2_dsra_tail_bwd(C.byref(d), ptr(mask), ptr(weit), ptr(wsum), ptr(sums), 1.0, None, 0, st)
        torch.cuda.synchronize()
        for j in range(2 * P):
            print(f"band {band} map {j}: relmax {relmax(lat[j], ups32[j]):.2e}")
            assert relmax(lat[j], ups32[j]) < 2e-6, (band, j)
        total = float(sum(ref_losses).detach())
        for j in range(P):
            ref = float(ref_losses[j].detach())
            print(f"band {band} loss {j}: {float(loss[j]):.7f} ref {ref:.7f}")
            assert abs(float(loss[j]) - ref) < 5e-6 * abs(ref), (band, j)
        assert abs(float(loss[P]) - total) < 5e-6 * abs(total), band
        for j in range(2 * P):
            got = dsrcs[j] - base[j] if j % 3 == 0 else dsrcs[j]
            print(f"band {band} grad {j}: relmax {relmax(got, ref_grads[j]):.2e} rell2 {rell2(got, ref_grads[j]):.2e}")
            assert relmax(got, ref_grads[j]) < 2e-4 and rell2(got, ref_grads[j]) < 2e-5, (band, j)


@pytest.mark.parametrize("wide", [False, True], ids=["ld=K", "ld=16"])
@pytest.mark.parametrize("K", [5, 13])
def test_fused_labels_with_five_and_thirteen_classes(K, wide):
    """pn2_seg_labels_up with (K + 3) / 4 = 2 and 4 channel vectors per pixel, scalar reads (ld = K, odd) and 16-byte reads (ld = 16), every mode, two samples of
    32 x 32 labels from maps at 1/32 .. 1/4: byte for byte against seglabelupref on dyadic maps, where every float32 intermediate is exact."""
    from pn2 import capi
    from pn2.capi import call
    N, OH, OW = 2, 32, 32
    ld = 16 if wide else K
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for mode in R.MODES:
        nmaps, scales = R.case(mode)
        maps = R.dyadic_maps(K, ld, [(OH // s, OW // s) for s in scales], N, seed=100 * K + ld + nmaps)
        dmaps = [torch.from_numpy(m).to(dev) for m in maps]
        table = (capi.SegUpMap * nmaps)()
        for i, t in enumerate(dmaps):
            table[i].p, table[i].ld, table[i].H, table[i].W = t.data_ptr(), ld, t.shape[1], t.shape[2]
        out = torch.full((N, OH, OW), 255, dtype=torch.uint8, device=dev)
        call.pn2_seg_labels_up(table, nmaps, R.MODES[mode], N, K, OH, OW, C.c_void_p(out.data_ptr()), st)
        torch.cuda.synchronize()
        assert R.tie_share(maps, scales, mode, K) > 0
        assert np.array_equal(out.cpu().numpy(), R.labels(maps, scales, mode, K)), mode
