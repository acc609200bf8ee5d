"""CPU tests of the ragged-batch input transform: the numpy restatement tests/inputbatchref.py against the oracle and Pillow's stored outputs, the pure-numpy
table and arena builders of pn2/input.py, and the refusal codes of pn2_input_batch_width / pn2_input_batch_height (decided on the host: no device is touched)."""
import ctypes as C
import os

import numpy as np
import pytest

import inputbatchref as R
from oracle import input_oracle as I

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fixtures():
    z = np.load(os.path.join(G, "input_pipeline.npz"))
    return z, sorted({k.split(".")[0] for k in z.files})


def test_ref_equals_oracle_and_pillow_on_every_fixture():
    """Every image and mask of input_pipeline.npz, batched per output size: the bytes equal Pillow's stored ones and the oracle's, the fp32 samples equal the stored
    tensors and the oracle's train_transform bit for bit (images normalised, masks not)."""
    from pn2.input import TapArena, batch_table
    z, names = _fixtures()
    by_size = {}
    for n in names:
        by_size.setdefault(z[n + ".resized"].shape[0], []).append(n)
    assert 352 in by_size and len(names) == 7
    for S, group in sorted(by_size.items()):
        arrs = [z[n + ".in"] if z[n + ".in"].ndim == 3 else z[n + ".in"][:, :, None] for n in group]
        taps = TapArena(S)
        rows, src_bytes, tmp_bytes = batch_table([a.shape for a in arrs], S, taps)
        src = R.pack(arrs, rows, src_bytes)
        n_rgb, n_mask = sum(a.shape[2] == 3 for a in arrs), sum(a.shape[2] == 1 for a in arrs)
        tmp, out_rgb, out_mask = R.run(rows, src, taps.data, S, tmp_bytes, n_rgb, n_mask)
        for n, a, r, b in zip(group, arrs, rows, R.height_bytes(rows, tmp, taps.data, S)):
            pil = z[n + ".resized"].reshape(S, S, -1)
            assert np.array_equal(b, pil), n
            assert np.array_equal(b, I.pil_resize_bilinear_u8(a, S, S)), n
            got = (out_rgb if a.shape[2] == 3 else out_mask)[int(r["dst"])]
            if a.shape[2] == 3:
                want = I.train_transform(a, a[:, :, 0], S)[0]
            else:
                want = I.train_transform(np.repeat(a, 3, axis=2), a[:, :, 0], S)[1]
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), n
            if n + ".tensor" in z.files:
                assert np.array_equal(got.view(np.uint32), z[n + ".tensor"].view(np.uint32)), n


def test_ref_copy_passes_and_empty_slot():
    """W == S and H == S are copies (no tap block is read: the arena holds none), an empty slot leaves its sample and every byte outside the slots as it was."""
    from pn2.input import TapArena, batch_table
    rng = np.random.default_rng(0)
    S = 12
    arrs = [rng.integers(0, 256, (12, 12, 3), dtype=np.uint8), None, rng.integers(0, 256, (12, 12, 1), dtype=np.uint8)]
    taps = TapArena(S)
    rows, src_bytes, tmp_bytes = batch_table([None if a is None else a.shape for a in arrs], S, taps, dst=[1, 0, 0], gap=5)
    assert taps.ints == 0 and taps.blocks == {}
    tmp, out_rgb, out_mask = R.run(rows, R.pack(arrs, rows, src_bytes), taps.data, S, tmp_bytes, 2, 1)
    assert np.array_equal(out_rgb[1], R.to_tensor(arrs[0], True)) and np.array_equal(out_mask[0], R.to_tensor(arrs[2], False))
    assert (out_rgb[0] == np.float32(-7.0)).all()
    live = np.zeros(tmp_bytes, bool)
    for r in rows:
        live[int(r["tmp"]):int(r["tmp"]) + int(r["H"]) * S * int(r["C"])] = True
    assert (tmp[~live] == 0xA5).all() and live.sum() == 12 * 12 * 4


def test_batch_table_layout():
    from pn2 import input as M
    from pn2.capi import call
    assert M.SLOT.itemsize == 64
    assert [M.SLOT.fields[n][1] for n in ("H", "W", "C", "dst", "norm", "kw", "kh", "blk", "src", "tmp", "tap_w", "tap_h")] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56]
    S = 32
    shapes = [(37, 53, 3), (32, 80, 3), None, (90, 32, 3), (53, 37, 1), (37, 53, 3), (0, 0, 3), (32, 32, 1)]
    taps = M.TapArena(S)
    for gap in (0, 7):
        rows, src_bytes, tmp_bytes = M.batch_table(shapes, S, taps, gap=gap)
        spans_s, spans_t, blk = [], [], 0
        for r, s in zip(rows, shapes):
            assert int(r["blk"]) == blk
            if s is None or s[0] == 0:
                assert int(r["H"]) == 0 and int(r["src"]) == 0 and int(r["tmp"]) == 0          # an empty slot: no bytes, no blocks
                continue
            H, W, Cc = s
            assert (int(r["H"]), int(r["W"]), int(r["C"])) == s and int(r["norm"]) == int(Cc == 3)
            assert int(r["src"]) % 16 == 0 and int(r["tmp"]) % 16 == 0
            spans_s.append((int(r["src"]), int(r["src"]) + H * W * Cc))
            spans_t.append((int(r["tmp"]), int(r["tmp"]) + H * S * Cc))
            assert int(r["kw"]) == (0 if W == S else call.pn2_resize_ksize(W, S)) and int(r["kh"]) == (0 if H == S else call.pn2_resize_ksize(H, S))
            assert slot_blocks_c(H, S) == M.slot_blocks(H, S)
            blk += M.slot_blocks(H, S)
        for spans, total in ((spans_s, src_bytes), (spans_t, tmp_bytes)):
            assert spans[0][0] >= gap and spans[-1][1] + gap <= total
            for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
                assert a1 + gap <= b0          # in slot order, never overlapping, the gap between them
        assert [int(r["dst"]) for r in rows if r["H"] > 0] == [0, 1, 2, 0, 3, 1]          # images and masks each count from 0
        # a repeated size shares one tap block; both axes of one length share it too
        assert rows[0]["tap_w"] == rows[5]["tap_w"] and rows[0]["tap_h"] == rows[5]["tap_h"] and rows[0]["tap_w"] == rows[4]["tap_h"] and rows[0]["tap_h"] == rows[4]["tap_w"]
    assert sorted(taps.blocks) == [37, 53, 80, 90]          # 32 needs none; the second table added nothing
    dst = M.batch_table(shapes, S, taps, dst=[5, 4, 0, 3, 2, 1, 0, 0], norm=[0, 1, 0, 0, 1, 1, 0, 0])[0]
    assert [int(r["dst"]) for r in dst] == [5, 4, 0, 3, 2, 1, 0, 0] and [int(r["norm"]) for r in dst] == [0, 1, 0, 0, 1, 1, 0, 0]
    with pytest.raises(ValueError):
        M.batch_table([(4, 4, 2)], S, taps)
    with pytest.raises(ValueError):
        M.batch_table([(4, 4, 3)], 16, taps)


def slot_blocks_c(rows, S):
    from pn2.capi import call
    return int(call.pn2_input_batch_blocks(rows, S))


def test_tap_arena_equals_resize_coeffs_per_size():
    from pn2.input import TapArena
    from pn2.capi import call
    for S in (32, 44):
        taps = TapArena(S)
        sizes = [53, 7, 200, 1, 53, 150, 5]
        offs = [taps.get(n) for n in sizes]
        assert offs[0] == offs[4] and len(taps.blocks) == 6
        end = 0
        for n, (off, ks) in zip(sizes, offs):
            assert ks == call.pn2_resize_ksize(n, S)
            xmin, cnt, kk = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros((S, ks), np.int32)
            call.pn2_resize_coeffs(n, S, C.c_void_p(xmin.ctypes.data), C.c_void_p(cnt.ctypes.data), C.c_void_p(kk.ctypes.data))
            gx, gc, gk = R.tap_views(taps.data, off, S, ks)
            assert np.array_equal(gx, xmin) and np.array_equal(gc, cnt) and np.array_equal(gk, kk)
            ox, oc, ok = I.resize_coeffs(n, S)
            assert np.array_equal(gx, ox) and np.array_equal(gc, oc) and np.array_equal(gk, ok)
            end = max(end, off + 2 * S + S * ks)
        assert taps.ints == end == sum(2 * S + S * ks for _, ks in set(offs))          # back to back, nothing twice


def test_batch_entries_refuse_on_the_host():
    """-1: null pointer, n < 0, out_size < 1; -2: C outside {1, 3}; -3: a row that disagrees with the arenas; n == 0: success.  The pointers are host addresses that
    no kernel ever sees: every one of these calls returns before a launch."""
    from pn2 import capi
    from pn2.input import TapArena, batch_table
    lib = capi.load()
    S = 32
    taps = TapArena(S)
    rows, src_bytes, tmp_bytes = batch_table([(37, 53, 3), (20, 32, 1)], S, taps)
    one = np.zeros(64, np.uint8)
    P = lambda a: C.c_void_p(a.ctypes.data)

    def width(rows=rows, **k):
        d = dict(th=P(rows), td=P(one), n=len(rows), S=S, src=P(one), src_bytes=src_bytes, tmp=P(one), tmp_bytes=tmp_bytes, taps=P(one), tap_ints=taps.ints, st=None)
        d.update(k)
        return lib.pn2_input_batch_width(*d.values())

    def height(rows=rows, **k):
        d = dict(th=P(rows), td=P(one), n=len(rows), S=S, tmp=P(one), tmp_bytes=tmp_bytes, taps=P(one), tap_ints=taps.ints, rgb=P(one), n_rgb=1, mask=P(one), n_mask=1,
                 mean=P(one), std=P(one), st=None)
        d.update(k)
        return lib.pn2_input_batch_height(*d.values())
    for f in (width, height):
        assert f(th=None) == -1 and f(td=None) == -1 and f(tmp=None) == -1 and f(taps=None) == -1 and f(n=-1) == -1 and f(S=0) == -1 and f(S=-4) == -1
        assert f(n=0) == 0 and f(n=0, S=0) == -1
        for Cc in (0, 2, 4):
            bad = rows.copy()
            bad[1]["C"] = Cc
            assert f(rows=bad) == -2, Cc
        for field, v in (("tmp", tmp_bytes), ("tmp", -16), ("blk", 3)):
            bad = rows.copy()
            bad[1][field] = v
            assert f(rows=bad) == -3, field
    assert width(src=None) == -1 and height(mean=None) == -1 and height(std=None) == -1 and height(rgb=None) == -1 and height(mask=None) == -1
    for field, v in (("src", src_bytes), ("kw", 3), ("tap_w", taps.ints)):
        bad = rows.copy()
        bad[0][field] = v
        assert width(rows=bad) == -3, field
    for field, v in (("dst", 1), ("dst", -1), ("kh", 9), ("tap_h", -1)):
        bad = rows.copy()
        bad[0][field] = v
        assert height(rows=bad) == -3, field
    assert lib.pn2_input_batch_blocks(-1, 32) == -1 and lib.pn2_input_batch_blocks(5, 0) == -1 and lib.pn2_input_batch_blocks(0, 32) == 0
    assert lib.pn2_input_batch_blocks(37, 32) == 2 and lib.pn2_input_batch_blocks(32, 30) == 1 and lib.pn2_input_batch_blocks(33, 30) == 2
