"""tests/raggedref.py against live scipy.ndimage on the ragged cases the GPU tests use, bit for bit; the committed fixture tests/golden/acdc_ragged.npz against
raggedref; and the host half of the ragged entry points of csrc/pn2_zoom.hip without a GPU: the planner's offsets, swapped shapes, copy flags, shared tables,
block tables and refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import raggedref as R
import zoomref as Z

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = list(R.BATCHES) + ["one"]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _case(name):
    return R.batch_inputs(R.ONE if name == "one" else name)


# ------------------------------------------------------------------------------------------------ the restatement against scipy
@pytest.mark.parametrize("name", CASES)
def test_ragged_generator_equals_the_loader(name):
    nd = pytest.importorskip("scipy.ndimage")
    images, labels, draws, size = _case(name)
    got = R.random_generator(images, labels, size, draws)
    assert got["image"].shape == (len(images), 1) + size and got["image"].dtype == np.float32 and got["label"].shape == (len(images),) + size and got["label"].dtype == np.int64
    for i, (im, lb, d) in enumerate(zip(images, labels, draws)):
        if d and d[0] == "rot_flip":          # dataset_ACDC.py:13-20
            im, lb = np.flip(np.rot90(im, d[1]), axis=d[2]).copy(), np.flip(np.rot90(lb, d[1]), axis=d[2]).copy()
        elif d:          # :23-27
            im, lb = nd.rotate(im, d[1], order=0, reshape=False), nd.rotate(lb, d[1], order=0, reshape=False)
        x, y = im.shape
        if x != size[0] or y != size[1]:          # :41-44
            im, lb = nd.zoom(im, (size[0] / x, size[1] / y), order=3), nd.zoom(lb, (size[0] / x, size[1] / y), order=0)
        assert im.shape == size, (i, im.shape)
        assert _same(got["image"][i, 0], im.astype(np.float32)), (name, i, d)
        assert np.array_equal(got["label"][i], lb.astype(np.float32).astype(np.int64)), (name, i, d)


def test_val_zooms_equal_scipy():
    nd = pytest.importorskip("scipy.ndimage")
    images, _, _, size = _case("zero_row")
    got = R.zoom_ragged(images, size, 3)
    for g, im in zip(got, images):
        x, y = im.shape
        want = im if (x, y) == size else nd.zoom(im, (size[0] / x, size[1] / y), order=3)
        assert _same(g, want)
    maps, sizes = R.unzoom_inputs()
    for g, m, s in zip(R.unzoom_labels(maps, sizes), maps, sizes):
        want = m if m.shape == s else nd.zoom(m, (s[0] / m.shape[0], s[1] / m.shape[1]), order=0)
        assert want.shape == s and _same(g, want)


def test_fixture_holds_what_raggedref_computes():
    G = np.load(os.path.join(HERE, "golden", "acdc_ragged.npz"))
    for name in R.BATCHES:
        images, labels, draws, size = R.batch_inputs(name)
        want = R.random_generator(images, labels, size, draws)
        assert _same(G[name + "/image"], want["image"][:, 0]) and _same(G[name + "/label"], want["label"].astype(np.uint8)), name
    maps, sizes = R.unzoom_inputs()
    for i, w in enumerate(R.unzoom_labels(maps, sizes)):
        assert _same(G[f"unzoom/{i}"], w)
    # the zero edges scipy leaves: the last row of 64 -> 28, the last column of 28 -> 48; 48 -> 28 has none
    zr, zc = G["zero_row/image"], G["zero_col/image"]
    assert not zr[0, -1].any() and zr[0, :-1, -1].any() and not zr[1, -1].any() and not zr[2, :, -1].any() and zr[2, -1, :-1].any()
    assert not zc[0, :, -1].any() and zc[0, -1, :-1].any()


def test_dice_is_medpys():
    g = np.random.default_rng(3)
    a, b = g.integers(0, 4, (33, 17)).astype(np.uint8), g.integers(0, 4, (33, 17)).astype(np.uint8)
    i, p, q = R.dice_counts(a, b)
    assert (i, p, q) == (int(((a > 0) & (b > 0)).sum()), int((a > 0).sum()), int((b > 0).sum())) and R.dc(a, b) == 2.0 * i / (p + q)
    z = np.zeros((5, 7), np.uint8)
    assert R.dc(z, z) == 0.0 and R.dc(a, np.zeros_like(a)) == 0.0 and R.dc(a, a) == 1.0


# ------------------------------------------------------------------------------------------------ the planner (host code)
def _plan(shapes, sizes, draws=None, offsets=None):
    from pn2 import volinput as V
    return V.RaggedPlan(V.ragged_samples(shapes, sizes, draws, offsets), packed=offsets is None)


def _table(plan, off, nout, order):
    """The (idx, w, valid) of one axis table of a plan, as pn2_zoom_tables lays them out."""
    h = plan.header
    tab = plan.host[h.tab_off:].view(np.float64)
    if order == 3:
        w = tab[off:off + 4 * nout].reshape(nout, 4)
        idx = tab[off + 4 * nout:off + 6 * nout].view(np.int32).reshape(nout, 4)
        return idx, w, idx[:, 0] >= 0
    idx = tab[off:off + (nout + 1) // 2].view(np.int32)[:nout]
    return idx, None, idx >= 0


@pytest.mark.parametrize("name", CASES)
def test_plan_describes_the_batch(name):
    images, _, draws, size = _case(name)
    shapes = [im.shape for im in images]
    plan = _plan(shapes, size, draws)
    h, src, work, out, b0, b1 = plan.header, 0, 0, 0, [0], [0]
    assert h.N == len(shapes) and h.uniform_out == 1 and h.max_out == size[0] * size[1] and h.bytes == plan.host.size
    for (H, W), d, dr in zip(shapes, plan.descs, draws):
        swap = dr is not None and dr[0] == "rot_flip" and dr[1] % 2 == 1
        gh, gw = (W, H) if swap else (H, W)
        assert (d.H, d.W, d.gh, d.gw, d.oh, d.ow) == (H, W, gh, gw) + size, (name, H, W, dr)
        assert d.geom == (0 if dr is None else 1 if dr[0] == "rot_flip" else 2)
        if d.geom == 1:
            assert (d.k, d.axis) == (dr[1], dr[2])
        if d.geom == 2:
            assert tuple(d.m6) == Z.rotate_matrix(dr[1], H, W)
        assert d.copy == int((gh, gw) == size)
        assert (d.src_off, d.lab_off, d.out_off) == (src, src, out)
        assert np.float64(d.zn0).view(np.uint64) == np.float64(Z.pole_pow(gh)).view(np.uint64) and np.float64(d.zn1).view(np.uint64) == np.float64(Z.pole_pow(gw)).view(np.uint64)
        src, out = src + H * W, out + size[0] * size[1]
        b0.append(b0[-1] + (0 if d.copy else (gw + 63) // 64))
        b1.append(b1[-1] + (0 if d.copy else (gh + 63) // 64))
        if d.copy:
            continue
        assert d.work_off == work
        work += gh * gw
        for off3, off0, nin, nout in ((d.ty3, d.ty0, gh, size[0]), (d.tx3, d.tx0, gw, size[1])):
            idx, w, valid = _table(plan, off3, nout, 3)
            ridx, rw, rvalid = Z.tables3(nin, nout)
            assert np.array_equal(valid, rvalid) and np.array_equal(idx[valid], ridx[valid]) and np.array_equal(w[valid].view(np.uint64), rw[valid].view(np.uint64))
            assert idx[valid].min() >= 0 and idx.max() <= nin - 1
            idx, _, valid = _table(plan, off0, nout, 0)
            ridx, rvalid = Z.tables0(nin, nout)
            assert np.array_equal(valid, rvalid) and np.array_equal(idx[valid], ridx[valid]) and idx.max() <= nin - 1
    assert (h.src_elems, h.work_doubles, h.out_elems) == (src, work, out)
    got0, got1 = plan.block_starts()
    assert got0.tolist() == b0 and got1.tolist() == b1 and (h.blocks0, h.blocks1) == (b0[-1], b1[-1])


def test_plan_shares_tables_and_sizes_the_workspace():
    # three samples of two distinct (nin, nout) per axis and order: 2 x 2 x 2 tables, not 3 x 4
    plan = _plan([(40, 56), (40, 56), (48, 56)], (28, 28))
    a, b, c = plan.descs
    assert (a.ty3, a.tx3, a.ty0, a.tx0) == (b.ty3, b.tx3, b.ty0, b.tx0) and c.tx3 == a.tx3 and c.tx0 == a.tx0 and c.ty3 != a.ty3 and c.ty0 != a.ty0
    assert plan.header.ntables == 6 and len({a.ty3, a.tx3, a.ty0, a.tx0, c.ty3, c.ty0}) == 6
    assert plan.header.bytes == plan.header.tab_off + 8 * (3 * 6 * 28 + 3 * 14)
    # an odd-k swap makes (56, 40) the same axes as (40, 56)
    plan = _plan([(40, 56), (56, 40)], (28, 28), [None, ("rot_flip", 3, None)])
    assert (plan.descs[1].gh, plan.descs[1].gw, plan.descs[1].axis) == (40, 56, -1) and plan.descs[1].ty3 == plan.descs[0].ty3 and plan.header.ntables == 4
    # every sample already at its size: no tables, no blocks, no workspace; per-sample output sizes pack back to back
    plan = _plan([(5, 7), (9, 3)], [(5, 7), (9, 3)])
    h = plan.header
    assert (h.ntables, h.blocks0, h.blocks1, h.work_doubles, h.uniform_out, h.max_out, h.out_elems) == (0, 0, 0, 0, 0, 35, 62) and h.bytes == h.tab_off
    assert [d.out_off for d in plan.descs] == [0, 35] and all(d.copy for d in plan.descs)
    # offsets given: taken as they are, also negative ones
    plan = _plan([(5, 7), (9, 3)], (4, 4), offsets=[(128, 64), (-256, -32)])
    assert [(d.src_off, d.lab_off) for d in plan.descs] == [(128, 64), (-256, -32)] and plan.header.src_elems == 0


def test_plan_refusals():
    from pn2 import capi
    from pn2 import volinput as V
    lib = capi.load()
    n = C.c_longlong(0)
    buf = np.zeros(1 << 16, np.uint8)
    bp = C.c_void_p(buf.ctypes.data)

    def arr(*ss):
        return (capi.RaggedSample * len(ss))(*ss)
    ok = capi.RaggedSample(H=8, W=9, oh=4, ow=5, axis=-1)
    assert lib.pn2_ragged_plan_bound(1, arr(ok), C.byref(n)) == 0 and n.value >= 80 + 152 + 16 + 8 * (6 * 9 + 2 + 3)
    assert lib.pn2_ragged_plan(1, arr(ok), 1, bp, buf.size) == 0
    assert lib.pn2_ragged_plan(1, arr(ok), 1, bp, 100) == -4 and lib.pn2_ragged_plan(1, None, 1, bp, buf.size) == -1 and lib.pn2_ragged_plan(1, arr(ok), 1, None, buf.size) == -1
    assert lib.pn2_ragged_plan(0, arr(ok), 1, bp, buf.size) == -2 and lib.pn2_ragged_plan(capi.RAGGED_MAX_N + 1, arr(ok), 1, bp, buf.size) == -2
    assert lib.pn2_ragged_plan_bound(capi.RAGGED_MAX_N + 1, arr(ok), C.byref(n)) == -2
    for bad in (dict(H=1025), dict(W=0), dict(oh=1025), dict(ow=0)):
        s = capi.RaggedSample(**{**dict(H=8, W=9, oh=4, ow=5, axis=-1), **bad})
        assert lib.pn2_ragged_plan(1, arr(s), 1, bp, buf.size) == -2, bad
    for bad in (dict(geom=3), dict(geom=-1), dict(geom=1, k=4), dict(geom=1, k=1, axis=2), dict(geom=1, k=1, axis=-2)):
        s = capi.RaggedSample(**{**dict(H=8, W=9, oh=4, ow=5, axis=-1), **bad})
        assert lib.pn2_ragged_plan(1, arr(s), 1, bp, buf.size) == -3, bad
    # the launchers refuse a null pointer and a blob that is not a plan before any launch
    one = C.c_void_p(16)
    junk = np.zeros(256, np.uint8)
    jp = C.c_void_p(junk.ctypes.data)
    assert lib.pn2_ragged_prefilter(None, bp, one, one, None) == -1 and lib.pn2_ragged_prefilter(one, jp, one, one, None) == -2
    assert lib.pn2_ragged_zoom3(one, bp, one, one, None, None) == -1 and lib.pn2_ragged_zoom3(one, jp, one, one, one, None) == -2
    assert lib.pn2_ragged_zoom0(one, bp, None, one, None) == -1 and lib.pn2_ragged_zoom0(one, jp, one, one, None) == -2
    assert lib.pn2_ragged_dice_counts(one, None, bp, one, one, None) == -1 and lib.pn2_ragged_dice_counts(one, one, jp, one, one, None) == -2
    with pytest.raises(ValueError, match="1024"):
        V.ragged_samples([(8, 1025)], (4, 4))
    with pytest.raises(ValueError, match="1024"):
        V.ragged_samples([(8, 8)], (1025, 4))
    with pytest.raises(ValueError):
        V.ragged_samples([(8, 8)], (4, 4), [("shear", 1)])
    with pytest.raises(ValueError):
        V.RaggedPlan([])


def test_no_cpu_fallback():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from pn2 import volinput as V
    from pn2 import voleval as E
    f, u = np.zeros((8, 9), np.float32), np.zeros((8, 9), np.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.zoom_ragged([f], (4, 4), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.RaggedSliceTransform((4, 4))([f], [u], [None])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.unzoom_labels(torch.zeros(1, 4, 4, dtype=torch.uint8), [(8, 9)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.dice_counts(torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8), [(2, 2)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.val_slices([f], [u], None, 4, "last")
