"""GPU tests of the dual-supervision loss kernels for 2..9 classes and every supervision mode (pn2_dual_loss_fwd / _bwd behind pn2.loss.mutation_loss): against
float64 (tests/duallossref.py), maps outside every subset, an empty target class, bit identity with the K = 9 entry points, refusals, and the single-supervision
loss as their foreground half.

Shapes: 3 x 20 x 27 = 1620 pixels is 6 full blocks of 256 + a block of 84 = 5 full 16-lane rows + a row of 4 (tail block, partial DPP row, partial wave);
1 x 4 x 4 is one block, one DPP row, 240 idle lanes."""
import ctypes as C

import pytest
import torch

import duallossref as D

pytestmark = pytest.mark.gpu
dev = "cuda"


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()


def relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _inputs(N, K, H, W, seed, label=None, random_mask=False):
    g = torch.Generator().manual_seed(seed * 100 + K)
    maps = [torch.randn(N, K, H, W, generator=g) * 1.5 for _ in range(8)]
    if label is None:
        label = torch.randint(0, K, (N, H, W), generator=g)
    bg = torch.randint(0, 2, (N, K, H, W), generator=g).float() if random_mask else D.bg_mask_of(label, K)
    return maps, label, bg


def _run(maps, label, bg, mode, lc):
    from pn2.loss import mutation_loss
    leaves = [m.to(dev).requires_grad_(True) for m in maps]
    loss = mutation_loss(leaves, label.to(dev), bg.to(dev), lc, supervision=mode)
    loss.backward()
    return loss.detach(), [m.grad for m in leaves]


def _loss_case(N, K, H, W, mode, lc=D.LC, seed=3, label=None, random_mask=False):
    """mutation_loss + backward on random maps against tests/duallossref.py in float64: loss within 1e-5 relative, every used map's gradient (fg and bg) within
    2e-5 relmax (the bounds of test_mutation_loss_kernels_vs_reference_formula and of the single-loss _loss_case: same arithmetic, same scale); a map outside
    every subset has a gradient of exact zeros."""
    maps, label, bg = _inputs(N, K, H, W, seed, label, random_mask)
    loss, grads = _run(maps, label, bg, mode, lc)
    m64 = [m.double().requires_grad_(True) for m in maps]
    ref = D.dual_loss_ref(m64, label, bg.double(), mode, lc)
    ref.backward()
    used = {i for s in D.R.subsets(mode) for i in s}
    err = abs(float(loss) - float(ref)) / abs(float(ref))
    gerr = [relmax(g, b.grad) if i % 4 in used else float(g.abs().max()) for i, (g, b) in enumerate(zip(grads, m64))]
    print(f"\nmutation_loss K={K} {mode} {N}x{H}x{W}: loss rel err {err:.2e}, gradient relmax / |unused|max {' '.join(f'{v:.2e}' for v in gerr)}")
    assert err < 1e-5
    for i, (g, b) in enumerate(zip(grads, m64)):
        if i % 4 in used:
            assert gerr[i] < 2e-5, i
        else:
            assert b.grad is None and int(torch.count_nonzero(g)) == 0, i


@pytest.mark.parametrize("K", [2, 3, 4, 5, 6, 7, 8, 9])
def test_dual_loss_mutation_vs_float64(K):
    _loss_case(3, K, 20, 27, "mutation")


@pytest.mark.parametrize("mode", ["deep_supervision", "last"])
@pytest.mark.parametrize("K", [2, 4, 9])
def test_dual_loss_other_modes_vs_float64(K, mode):
    _loss_case(3, K, 20, 27, mode)


def test_dual_loss_random_background_mask_and_other_weights():
    """bg_mask a random 0/1 mask unrelated to the label, lc away from the defaults."""
    _loss_case(3, 4, 20, 27, "mutation", lc=(0.4, 0.9, 0.2), random_mask=True)


def test_dual_loss_single_partial_row():
    _loss_case(1, 9, 4, 4, "mutation")
    _loss_case(1, 4, 4, 4, "deep_supervision")


def test_dual_loss_empty_target_class():
    """K = 4 with labels that never take class 3: Dice with an empty target class (T = 0, the intersect sum exactly 0)."""
    label = torch.randint(0, 3, (3, 20, 27), generator=torch.Generator().manual_seed(11))
    assert int((label == 3).sum()) == 0
    _loss_case(3, 4, 20, 27, "mutation", label=label)


def test_dual_loss_unused_maps():
    """'deep_supervision' uses every map; in 'last' maps 0..2 (fg and bg) are outside the only subset: zero gradients (checked in _loss_case), and NaNs in them
    change neither the loss nor the used maps' gradients by a bit."""
    assert {i for s in D.R.subsets("deep_supervision") for i in s} == {0, 1, 2, 3}
    maps, label, bg = _inputs(3, 4, 20, 27, 5)
    loss, grads = _run(maps, label, bg, "last", D.LC)
    poisoned = [torch.full_like(m, float("nan")) if i % 4 < 3 else m for i, m in enumerate(maps)]
    loss_n, grads_n = _run(poisoned, label, bg, "last", D.LC)
    assert bool(torch.isfinite(loss)) and torch.equal(loss, loss_n)
    for i in range(8):
        if i % 4 == 3:
            assert float(grads[i].abs().max()) > 0 and torch.equal(grads[i], grads_n[i]), i
        else:
            assert int(torch.count_nonzero(grads[i])) == 0 and int(torch.count_nonzero(grads_n[i])) == 0, i


def _capi_pair(new, maps, label, bg, subsets=0x7FFF, lc=D.LC):
    """loss, sums and the eight gradients of one forward + backward through the C entry points (new: pn2_dual_loss_*, else pn2_mutation_loss_*)."""
    from pn2 import capi
    lib = capi.load()
    N, H, W, K = maps[0].shape
    P = lambda t: C.c_void_p(t.data_ptr())
    PA = C.c_void_p * 4
    wd = lib.pn2_dual_loss_width(K) if new else lib.pn2_mutation_loss_width(K)
    partial = torch.empty(lib.pn2_mutation_loss_blocks(N * H * W), wd, device=dev); sums = torch.empty(wd, device=dev); loss = torch.empty(1, device=dev)
    grads = [torch.full_like(m, 7.0) for m in maps]
    fg, bgp, dfg, dbg = (PA(*[t.data_ptr() for t in ts]) for ts in (maps[:4], maps[4:], grads[:4], grads[4:]))
    if new:
        rf = lib.pn2_dual_loss_fwd(fg, bgp, subsets, P(label), P(bg), N, H * W, K, *lc, P(partial), P(sums), P(loss), None)
        rb = lib.pn2_dual_loss_bwd(fg, bgp, dfg, dbg, subsets, P(label), P(bg), N, H * W, K, *lc, P(sums), 1.0, None)
    else:
        rf = lib.pn2_mutation_loss_fwd(fg, bgp, P(label), P(bg), N, H * W, K, *lc, P(partial), P(sums), P(loss), None)
        rb = lib.pn2_mutation_loss_bwd(fg, bgp, dfg, dbg, P(label), P(bg), N, H * W, K, *lc, P(sums), 1.0, None)
    torch.cuda.synchronize()
    assert rf == 0 and rb == 0, (rf, rb)
    return loss, sums, grads


@pytest.mark.parametrize("shape", [(3, 20, 27), (1, 4, 4)])
def test_dual_loss_k9_all_subsets_is_bit_identical_to_the_k9_entry_points(shape):
    """pn2_dual_loss_* with K = 9 / 0x7FFF against pn2_mutation_loss_* on the same buffers: loss, sums and the eight gradients, and two calls of the new path.  The
    forward kernels differ (dloss_fwd_k<9> against mloss_fwd_k<9>).  For this one case the new backward entry launches mloss_bwd_k<9>, so the
    gradient half checks that routing; dloss_bwd_k<9> itself is checked against float64 below and in the other two modes above."""
    N, H, W = shape
    maps, label, bg = _inputs(N, 9, H, W, 7)
    maps = [m.permute(0, 2, 3, 1).contiguous().to(dev) for m in maps]          # [N][H][W][K]
    label, bg = label.to(dev), bg.to(dev).contiguous()
    a = _capi_pair(True, maps, label, bg)
    b = _capi_pair(False, maps, label, bg)
    c = _capi_pair(True, maps, label, bg)
    for x, y in ((a, b), (a, c)):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
        for i in range(8):
            assert torch.equal(x[2][i], y[2][i]), i
    assert bool(torch.isfinite(a[0])) and all(float(g.abs().max()) > 0 and float(g.abs().max()) < 7.0 for g in a[2])


def test_dual_loss_k9_fourteen_subsets_vs_float64():
    """K = 9 with every subset but {0} (mask 0x7FFE), through the entry points: the most subsets dloss_bwd_k<9> ever runs (all 15 go to mloss_bwd_k<9>).  Same
    bounds as _loss_case: loss within 1e-5 relative, the eight gradients within 2e-5 relmax of float64."""
    maps, label, bg = _inputs(3, 9, 20, 27, 13)
    nhwc = [m.permute(0, 2, 3, 1).contiguous().to(dev) for m in maps]
    loss, _, grads = _capi_pair(True, nhwc, label.to(dev), bg.to(dev).contiguous(), subsets=0x7FFE)
    m64 = [m.double().requires_grad_(True) for m in maps]
    ref = 0.0
    for s in range(2, 16):          # subset s sums the maps whose bit is set in s; its mask bit is s - 1
        iout = sum(m64[i] for i in range(4) if s >> i & 1); ibg = sum(m64[4 + i] for i in range(4) if s >> i & 1)
        ref = ref + D.LC[0] * torch.nn.functional.cross_entropy(iout, label) + D.LC[1] * D.E.dice_loss(iout, label, 9) \
            + D.LC[2] * torch.nn.functional.binary_cross_entropy_with_logits(ibg, bg.double())
    ref.backward()
    err = abs(float(loss) - float(ref)) / abs(float(ref))
    gerr = [relmax(g.permute(0, 3, 1, 2), b.grad) for g, b in zip(grads, m64)]
    print(f"\ndual loss K=9 mask 0x7FFE: loss rel err {err:.2e}, gradient relmax {' '.join(f'{v:.2e}' for v in gerr)}")
    assert err < 1e-5 and max(gerr) < 2e-5, (err, gerr)


def test_dual_loss_unselected_columns_are_zeros():
    """The sums row of 'last' at K = 4: the columns of subsets 1..7 and 9..15 are zeros, subset 8's and the label histogram are not."""
    maps, label, bg = _inputs(3, 4, 20, 27, 9)
    maps = [m.permute(0, 2, 3, 1).contiguous().to(dev) for m in maps]
    _, sums, _ = _capi_pair(True, maps, label.to(dev), bg.to(dev).contiguous(), subsets=0x80)
    Wd = 2 + 2 * 4
    row = sums.cpu().reshape(-1)
    for s in range(15):
        cols = row[s * Wd:(s + 1) * Wd]
        assert (int(torch.count_nonzero(cols)) == Wd) if s == 7 else (int(torch.count_nonzero(cols)) == 0), s
    assert float(row[15 * Wd:].sum()) == 3 * 20 * 27


def test_dual_loss_bad_arguments():
    """K = 1, K = 10 raise with the supported range; an unknown supervision name and seven maps raise ValueError; subsets = 0 and a bit above 15 come back with
    status -2 from the entry points (checked before any launch)."""
    from pn2 import capi
    from pn2.loss import mutation_loss
    lib = capi.load()
    lab = torch.zeros(1, 4, 4, dtype=torch.long, device=dev)
    for K in (1, 10):
        maps = [torch.zeros(1, K, 4, 4, device=dev) for _ in range(8)]
        with pytest.raises(RuntimeError, match="2 <= K <= 9"):
            mutation_loss(maps, lab, torch.zeros(1, K, 4, 4, device=dev))
    maps = [torch.zeros(1, 4, 4, 4, device=dev) for _ in range(8)]
    with pytest.raises(ValueError):
        mutation_loss(maps, lab, torch.zeros(1, 4, 4, 4, device=dev), supervision="powerset")
    with pytest.raises(ValueError):
        mutation_loss(maps[:7], lab, torch.zeros(1, 4, 4, 4, device=dev))
    K = 4
    grads = [torch.full_like(m, 7.0) for m in maps]
    wd = lib.pn2_dual_loss_width(K)
    partial = torch.zeros(lib.pn2_mutation_loss_blocks(16), wd, device=dev); sums = torch.zeros(wd, device=dev); loss = torch.full((1,), 7.0, device=dev)
    bgm = torch.zeros(1, K, 4, 4, device=dev)
    PA = C.c_void_p * 4
    pm, pg = PA(*[m.data_ptr() for m in maps[:4]]), PA(*[m.data_ptr() for m in grads[:4]])
    P = lambda t: C.c_void_p(t.data_ptr())
    for subsets, k in ((0, K), (0x8000, K), (0x7FFF, 1), (0x7FFF, 10)):
        assert lib.pn2_dual_loss_fwd(pm, pm, subsets, P(lab), P(bgm), 1, 16, k, 0.5, 0.7, 0.3, P(partial), P(sums), P(loss), None) == -2
        assert lib.pn2_dual_loss_bwd(pm, pm, pg, pg, subsets, P(lab), P(bgm), 1, 16, k, 0.5, 0.7, 0.3, P(sums), 1.0, None) == -2
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and all(float(g.min()) == 7.0 for g in grads)          # nothing ran


def test_dual_loss_foreground_half_is_the_single_loss():
    """K = 4 / deep_supervision with lc3 = 0 against seg_loss(fg maps, 'deep_supervision', (lc1, lc2)): the same sums through separate reductions (no bit identity
    asked): loss within 1e-6 relative, gradients within 2e-6 relmax."""
    from pn2.loss import seg_loss
    maps, label, bg = _inputs(3, 4, 20, 27, 21)
    lb, gb = _run(maps, label, bg, "deep_supervision", (0.5, 0.7, 0.0))
    a = [m.to(dev).requires_grad_(True) for m in maps[:4]]
    la = seg_loss(a, label.to(dev), "deep_supervision", (0.5, 0.7)); la.backward()
    assert abs(float(la) - float(lb)) <= 1e-6 * abs(float(lb)), (float(la), float(lb))
    for x, y in zip(a, gb[:4]):
        assert relmax(x.grad, y) <= 2e-6
    for y in gb[4:]:
        assert int(torch.count_nonzero(y)) == 0          # lc3 = 0: the BCE gradients are 0 * finite
