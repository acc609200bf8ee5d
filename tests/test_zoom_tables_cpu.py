"""The host half of csrc/pn2_zoom.hip without a GPU: the per-axis tables, z^(n-1) and the rotate matrices that decide bits on the device, against tests/zoomref.py
double for double; the size limits at the boundary; no CPU fallback."""
import ctypes as C

import numpy as np
import pytest
import torch

import zoomref as Z

AXES = sorted({(s[i], d[i]) for s, d in Z.SHAPES for i in (0, 1)} | {(40, 24), (96, 64), (80, 64), (64, 96), (64, 80), (1, 1), (1, 5), (5, 1), (1024, 1024), (512, 256), (512, 352)})


def _tables(nin, nout, order):
    from pn2.capi import call
    per = 4 if order == 3 else 1
    idx, w, valid = np.full(nout * per, -7, np.int32), np.full(nout * per, np.nan), np.full(nout, -7, np.int32)
    call.pn2_zoom_tables(nin, nout, order, C.c_void_p(idx.ctypes.data), C.c_void_p(w.ctypes.data), C.c_void_p(valid.ctypes.data))
    return idx.reshape(nout, per), w.reshape(nout, per), valid.astype(bool)


@pytest.mark.parametrize("nin,nout", AXES)
def test_tables_equal_the_restatement(nin, nout):
    idx, w, valid = _tables(nin, nout, 3)
    ridx, rw, rvalid = Z.tables3(nin, nout)
    assert np.array_equal(valid, rvalid)
    assert np.array_equal(idx[valid], ridx[valid]) and np.array_equal(w[valid].view(np.uint64), rw[valid].view(np.uint64))
    assert not idx[~valid].any() and not w[~valid].any()          # a row scipy leaves at cval carries no taps
    assert idx.min() >= 0 and idx.max() <= nin - 1
    idx, _, valid = _tables(nin, nout, 0)
    ridx, rvalid = Z.tables0(nin, nout)
    assert np.array_equal(valid, rvalid) and np.array_equal(idx[:, 0], ridx) and idx.min() >= 0 and idx.max() <= nin - 1


def test_the_zero_edges_are_in_the_tables():
    """(nout - 1) * ((nin - 1) / (nout - 1)) > nin - 1 in double for 512 -> 224, 64 -> 28 and 28 -> 48; not for 512 -> 256, 512 -> 352, 224 -> 512, 48 -> 28, 28 -> 64."""
    for nin, nout, zero in ((512, 224, True), (64, 28, True), (28, 48, True), (48, 28, False), (512, 256, False), (512, 352, False), (224, 512, False), (28, 64, False)):
        for order in (0, 3):
            valid = _tables(nin, nout, order)[2]
            assert valid[:-1].all() and bool(valid[-1]) != zero, (nin, nout, order)


def test_pole_power_is_the_c_librarys():
    from pn2.capi import call
    for n in list(range(1, 70)) + [100, 224, 512, 540, 566, 640, 1024]:
        zn = C.c_double(-1.0)
        call.pn2_zoom_pole_pow(n, C.byref(zn))
        assert np.float64(zn.value).view(np.uint64) == np.float64(Z.pole_pow(n)).view(np.uint64), n
    zn = C.c_double(0.0)
    call.pn2_zoom_pole_pow(640, C.byref(zn))
    assert zn.value == 0.0 or abs(zn.value) < 2.3e-308          # the 640-sample line of the GPU tests runs through denormal and zero powers


def test_rotate_matrices_equal_the_restatement():
    from pn2 import volinput as V
    for H, W in Z.ROTATE_SHAPES + [(40, 40), (224, 224), (512, 512)]:
        for a in Z.ANGLES:
            assert V._rotate_matrix(float(a), H, W) == Z.rotate_matrix(a, H, W), (H, W, a)
    assert V._rotate_matrix(0.0, 37, 41) == (1.0, 0.0, -0.0, 1.0, 0.0, 0.0)


def test_sizes_are_refused_at_the_boundary():
    from pn2 import capi
    lib = capi.load()
    one, n = C.c_void_p(16), C.c_longlong(0)
    assert lib.pn2_zoom_tables(1025, 8, 3, one, one, one) == -2 and lib.pn2_zoom_tables(8, 1025, 0, one, one, one) == -2 and lib.pn2_zoom_tables(8, 0, 0, one, one, one) == -2
    assert lib.pn2_zoom_tables(8, 8, 1, one, one, one) == -1 and lib.pn2_zoom_tables(8, 8, 3, one, None, one) == -1
    assert lib.pn2_zoom_workspace(1, 1025, 8, C.byref(n)) == -2 and lib.pn2_zoom_workspace(0, 8, 8, C.byref(n)) == -2
    assert lib.pn2_zoom_workspace(3, 96, 80, C.byref(n)) == 0 and n.value == 2 * 3 * 96 * 80 * 8
    assert lib.pn2_zoom_prefilter(one, 1, 8, 1025, one, None) == -2 and lib.pn2_zoom_prefilter(None, 1, 8, 8, one, None) == -1
    assert lib.pn2_zoom3_gather(one, 1, 8, 8, 1025, 8, one, one, one, one, one, one, one, None) == -2
    assert lib.pn2_zoom0(1, one, 1, 8, 8, 8, 1025, one, one, one, one, one, None) == -2 and lib.pn2_zoom0(2, one, 1, 8, 8, 4, 4, one, one, one, one, one, None) == -3
    assert lib.pn2_rotate0(4, one, 1, 1025, 8, one, one, None) == -2 and lib.pn2_rotate0(8, one, 1, 8, 8, one, one, None) == -3
    assert lib.pn2_rot_flip(1, one, 1, 1025, one, one, None) == -2 and lib.pn2_rot_flip(1, one, 1, 8, None, one, None) == -1


def test_no_cpu_fallback_and_argument_errors():
    from pn2 import volinput as V
    x = torch.zeros(2, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.zoom(x, (4, 4), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.rotate(x, [0, 0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.rot_flip(x, [0, 0], [0, 0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.SliceTransform((4, 4))(x, x.to(torch.uint8))


def test_draw_makes_the_loaders_calls_in_the_loaders_order():
    import random
    from pn2.volinput import SliceTransform
    random.seed(1234); np.random.seed(1234)
    got = SliceTransform.draw(64)
    random.seed(1234); np.random.seed(1234)
    want = []
    for _ in range(64):          # dataset_synapse.py:35-38 with random_rot_flip (:13,16) and random_rotate (:23) written out
        if random.random() > 0.5:
            k = np.random.randint(0, 4)
            want.append(("rot_flip", k, np.random.randint(0, 2)))
        elif random.random() > 0.5:
            want.append(("rotate", np.random.randint(-20, 20)))
        else:
            want.append(None)
    assert got == want and {None if d is None else d[0] for d in got} == {None, "rot_flip", "rotate"}
