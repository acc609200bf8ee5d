"""CPU tests of the augmented input transform: the numpy restatement tests/inputaugref.py against Pillow byte for byte (rotation, flips, then the whole
pipeline), pn2.input.rotate_coeffs against it, DeviceTransform.draw against the reference loader's way of drawing, and the refusal codes of
pn2_input_batch_width_aug (decided on the host: no device is touched)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from PIL import Image

import inputaugref as A
import inputbatchref as R

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = [(1, 9), (7, 5), (31, 47), (64, 64), (288, 384), (966, 1225)]          # (H, W)
FLIPS = [(False, False), (True, False), (False, True), (True, True)]


def _angles():
    rng = np.random.default_rng(90)
    return [90.0, -90.0, 0.0, 45.0, 1e-7, 89.99999, 180.0] + [float(v) for v in rng.uniform(-90.0, 90.0, 12)]


def _image(H, W, Cc, seed):
    a = np.random.default_rng(seed).integers(0, 256, (H, W, Cc), dtype=np.uint8)
    return a


@pytest.mark.parametrize("H,W", SIZES)
def test_ref_equals_pillow_rotate_and_flips(H, W):
    """Image.rotate(angle, NEAREST, expand=False) -> FLIP_TOP_BOTTOM -> FLIP_LEFT_RIGHT, byte for byte, for L and RGB, every flip combination, +-90 (a transpose
    in Pillow on the square image), 0 (a copy), 180 (a transpose), 45, 1e-7, 89.99999 and a dozen seeded angles - by both routes of inputaugref: the rotation's own
    integers with numpy flips, and the folded integers of the device table; pn2.input.rotate_coeffs returns those same integers and modes."""
    from pn2.input import rotate_coeffs
    for Cc in (1, 3):
        img = _image(H, W, Cc, H * 10 + Cc)
        pil = Image.fromarray(img[:, :, 0] if Cc == 1 else img)
        for angle in _angles():
            rot = pil.rotate(angle, Image.NEAREST, expand=False)
            base = np.asarray(rot).reshape(H, W, Cc)
            assert np.array_equal(A.rotate_flip(img, angle, False, False), base), (Cc, angle)
            for fv, fh in FLIPS:
                want = np.asarray(A.pil_rotate_flip(pil, angle, fv, fh)).reshape(H, W, Cc)
                if H * W <= 64 * 64:
                    assert np.array_equal(A.rotate_flip(img, angle, fv, fh), want), (Cc, angle, fv, fh)
                a, mode = A.rotate_coeffs(angle, fv, fh, H, W)
                assert np.array_equal(A.gather(img, a), want), (Cc, angle, fv, fh)
                assert mode == int(angle != 0.0 or fv or fh)
                assert rotate_coeffs(angle, fv, fh, H, W) == (tuple(a), mode), (angle, fv, fh)
                if mode == 0:
                    assert np.array_equal(want, img)


def test_rotate_coeffs_modes_and_table_row():
    from pn2 import input as M
    assert M.AUG.itemsize == 32 and [M.AUG.fields[n][1] for n in ("a", "mode", "reserved")] == [0, 24, 28]
    assert M.rotate_coeffs(0.0, False, False, 5, 7)[1] == 0 and M.rotate_coeffs(360.0, False, False, 5, 7)[1] == 0 and M.rotate_coeffs(-720.0, False, False, 5, 7)[1] == 0
    assert M.rotate_coeffs(0.0, True, False, 5, 7)[1] == 1 and M.rotate_coeffs(360.0, False, True, 5, 7)[1] == 1 and M.rotate_coeffs(1e-7, False, False, 5, 7)[1] == 1
    assert M.rotate_coeffs(0.0, False, False, 5, 7)[0] == (65536, 0, 32768, 0, 65536, 32768)
    # the flips alone are exact index reversals
    img = _image(5, 7, 3, 1)
    assert np.array_equal(A.gather(img, M.rotate_coeffs(0.0, True, False, 5, 7)[0]), img[::-1])
    assert np.array_equal(A.gather(img, M.rotate_coeffs(0.0, False, True, 5, 7)[0]), img[:, ::-1])
    # the largest axis the entry accepts: every sum of the slot stays inside int32 (inputaugref.gather asserts it) at the angles that push the corners furthest
    B = M.AUG_MAX_AXIS
    for angle in (45.0, -45.0, 90.0, -90.0, 30.0, 1e-7):
        for fv, fh in FLIPS:
            a = np.array(M.rotate_coeffs(angle, fv, fh, B, B)[0], dtype=np.int64)
            for x, y in ((0, 0), (B, 0), (0, B), (B, B)):
                for k in (0, 3):
                    v = int(a[k + 2] + a[k] * x + a[k + 1] * y)
                    assert A.I32[0] <= v <= A.I32[1], (angle, fv, fh, x, y)
    rows = M.aug_table([(5, 7, 3), None, (5, 7, 1), (0, 0, 3)], [(30.0, True, False), (30.0, True, False), None, (1.0, False, False)])
    assert [int(r["mode"]) for r in rows] == [1, 0, 0, 0] and tuple(int(v) for v in rows[0]["a"]) == A.rotate_coeffs(30.0, True, False, 5, 7)[0]
    with pytest.raises(ValueError):
        M.aug_table([(B + 1, 4, 3)], [(30.0, False, False)])


@pytest.mark.parametrize("H,W,S", [(97, 130, 32), (20, 24, 32), (64, 64, 64)])
def test_ref_whole_pipeline_equals_pillow(H, W, S):
    """Pillow rotate, flips and resize((S, S), BILINEAR), then ToTensor / Normalize in float32: the output bits of the reference's batch (second table, width pass
    through the map, height pass) for an image and its mask under one draw, next to a slot left in mode 0."""
    from pn2.input import TapArena, batch_table
    rng = np.random.default_rng(H)
    draws = [(float(rng.uniform(-90, 90)), True, False), (90.0, False, True), (-33.3, True, True), None]
    imgs = [_image(H, W, 3, 100 + i) for i in range(len(draws))]
    gts = [_image(H, W, 1, 200 + i) for i in range(len(draws))]
    arrs, per_slot = imgs + gts, draws + draws
    taps = TapArena(S)
    rows, src_bytes, tmp_bytes = batch_table([a.shape for a in arrs], S, taps)
    aug = A.aug_rows([a.shape for a in arrs], per_slot)
    assert [int(g["mode"]) for g in aug] == [1, 1, 1, 0] * 2
    _, out_rgb, out_mask = A.run(rows, aug, R.pack(arrs, rows, src_bytes), taps.data, S, tmp_bytes, len(imgs), len(gts))
    for i, d in enumerate(draws):
        want_x, want_g = A.pil_pipeline(imgs[i], d, S, True), A.pil_pipeline(gts[i][:, :, 0], d, S, False)
        assert np.array_equal(out_rgb[i].view(np.uint32), want_x.view(np.uint32)), (i, d)
        assert np.array_equal(out_mask[i].view(np.uint32), want_g.view(np.uint32)), (i, d)


def test_ref_reproduces_fixture():
    """input_aug.npz (made with Pillow alone, tests/golden/make_golden_input_aug.py) through the reference"""
    from pn2.input import TapArena, batch_table
    z = np.load(os.path.join(G, "input_aug.npz"))
    names = sorted({k.split(".")[0] for k in z.files})
    assert len(names) == 6
    for n in names:
        S = z[n + ".x"].shape[-1]
        d = (float(z[n + ".draw"][0]), bool(z[n + ".draw"][1]), bool(z[n + ".draw"][2]))
        arrs = [z[n + ".img"], z[n + ".gt"][:, :, None]]
        taps = TapArena(S)
        rows, src_bytes, tmp_bytes = batch_table([a.shape for a in arrs], S, taps)
        _, out_rgb, out_mask = A.run(rows, A.aug_rows([a.shape for a in arrs], [d, d]), R.pack(arrs, rows, src_bytes), taps.data, S, tmp_bytes, 1, 1)
        assert np.array_equal(out_rgb[0].view(np.uint32), z[n + ".x"].view(np.uint32)), n
        assert np.array_equal(out_mask[0].view(np.uint32), z[n + ".g"].view(np.uint32)), n


def test_draw_equals_the_loaders_draws_and_leaves_the_global_generator():
    """After np.random.seed(k): draw(n) is the sequence the reference loader gets by seeding torch's GLOBAL generator with np.random.randint(2147483647) per sample
    and making the three torchvision calls; the global generator's state is not touched by draw; seeding again (the loader does, before the mask's transforms)
    repeats the decisions, which is why image and mask share one draw."""
    from pn2.input import DeviceTransform
    for k in (0, 7):
        np.random.seed(k)
        torch.manual_seed(1234 + k)
        before = torch.get_rng_state()
        got = DeviceTransform.draw(5)
        assert torch.equal(torch.get_rng_state(), before)
        assert len(got) == 5 and all(isinstance(a, float) and -90.0 <= a <= 90.0 and isinstance(v, bool) and isinstance(h, bool) for a, v, h in got)
        np.random.seed(k)
        want = []
        for _ in range(5):
            seed = np.random.randint(2147483647)
            both = []
            for _ in ("image", "mask"):
                torch.manual_seed(seed)
                angle = float(torch.empty(1).uniform_(-90., 90.).item())
                fv = bool(torch.rand(1) < 0.5)
                fh = bool(torch.rand(1) < 0.5)
                both.append((angle, fv, fh))
            assert both[0] == both[1]
            want.append(both[0])
        assert got == want
        assert len({a for a, _, _ in got}) == 5
    assert DeviceTransform.draw(0) == []


def test_aug_entry_refuses_on_the_host():
    """-1: a null second table (either copy) and the first entry's own -1 cases; -3: a mode outside 0 and 1; -2: a mode-1 slot with an axis above
    PN2_INPUT_AUG_MAX_AXIS, or whose integers leave int32 at a corner - the same axis in mode 0 is accepted; n == 0: success.  The pointers are host addresses
    that no kernel ever sees: every one of these calls returns before a launch."""
    from pn2 import capi
    from pn2.input import AUG, AUG_MAX_AXIS, TapArena, batch_table, rotate_coeffs
    lib = capi.load()
    S = 32
    taps = TapArena(S)
    shapes = [(37, 53, 3), (20, 32, 1)]
    rows, src_bytes, tmp_bytes = batch_table(shapes, S, taps)
    aug = A.aug_rows(shapes, [(30.0, True, False), None])
    one = np.zeros(64, np.uint8)
    P = lambda a: C.c_void_p(a.ctypes.data)

    def f(rows=rows, aug=aug, **k):
        d = dict(th=P(rows), td=P(one), ah=P(aug), ad=P(one), n=len(rows), S=S, src=P(one), src_bytes=src_bytes, tmp=P(one), tmp_bytes=tmp_bytes, taps=P(one),
                 tap_ints=taps.ints, st=None)
        d.update(k)
        return lib.pn2_input_batch_width_aug(*d.values())
    assert f(ah=None) == -1 and f(ad=None) == -1
    assert f(th=None) == -1 and f(td=None) == -1 and f(src=None) == -1 and f(tmp=None) == -1 and f(taps=None) == -1 and f(n=-1) == -1 and f(S=0) == -1
    assert f(n=0) == 0 and f(n=0, ah=None) == -1
    for mode in (2, -1, 256):
        bad = aug.copy()
        bad[1]["mode"] = mode
        assert f(aug=bad) == -3, mode
    bad = rows.copy()
    bad[0]["blk"] = 3
    assert f(rows=bad) == -3          # the first table is checked as pn2_input_batch_width checks it
    # An axis above the bound is refused in mode 1 and accepted in mode 0.  An accepted batch would go on to a launch, which a host test must not reach: the
    # entry checks the second table first, so a wrong blk in a LATER row of the first table turns every batch the second table's check accepts into -3.
    B = AUG_MAX_AXIS
    on, off = np.zeros(2, AUG), np.zeros(2, AUG)
    on[0]["a"], on[0]["mode"] = (65536, 0, 32768, 0, 65536, 32768), 1
    for over, at in (((B + 1, 8, 1), (B, 8, 1)), ((8, B + 1, 1), (8, B, 1))):
        arena = TapArena(S)
        big, big_src, big_tmp = batch_table([over, None], S, arena)
        kw = dict(src_bytes=big_src, tmp_bytes=big_tmp, tap_ints=arena.ints)
        assert f(rows=big, aug=on, **kw) == -2, over
        big[1]["blk"] += 1
        assert f(rows=big, aug=on, **kw) == -2 and f(rows=big, aug=off, **kw) == -3, over          # mode 0: past the second table's check
        ok, ok_src, ok_tmp = batch_table([at, None], S, arena)
        ok[1]["blk"] += 1
        assert f(rows=ok, aug=on, src_bytes=ok_src, tmp_bytes=ok_tmp, tap_ints=arena.ints) == -3, at          # mode 1 at the bound: accepted too
    # integers that leave int32 inside the slot
    wild = aug.copy()
    wild[0]["a"] = (65536, 65536, (1 << 31) - 65536 * 60, 0, 65536, 32768)
    assert f(aug=wild) == -2
    wild[0]["mode"] = 0
    wild[1]["a"], wild[1]["mode"] = rotate_coeffs(-12.5, False, True, 20, 32)[0], 1
    empty = rows.copy()
    empty["H"] = 0
    empty["blk"] = 0
    assert f(rows=empty, aug=wild) == 0          # mode 0 ignores its integers; a batch of empty slots launches nothing
