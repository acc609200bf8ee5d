"""GPU tests of the augmented input transform: pn2_input_batch_width_aug (csrc/pn2_input.hip) through the C ABI with guard bytes around every arena, table and
output, against tests/inputaugref.py and Pillow bit for bit; its mode-0 slots against pn2_input_batch_width; then DeviceTransform.batch(draws=...) against the
Pillow-made fixture, its call pattern, and get_loader(augmentation=...)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import inputaugref as A
import inputbatchref as R

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
os.environ.setdefault("PN2_NO_PRETRAINED", "1")
CANARY = 0xA5
FILL = np.float32(-7.0)
GAP = 32          # guard bytes before every slot of the source / scratch arenas and after the last


def _dev():
    return torch.device("cuda", 0)


def _P(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_T = {}


def _transform(S):
    from pn2.input import DeviceTransform
    if S not in _T:
        _T[S] = DeviceTransform(S)
    return _T[S]


def _pairs():
    """(H, W, draw) of every image of the batch under test; its mask follows with the same size and draw.  None as a size: an empty slot; None as a draw: mode 0.
    7 x 5 and 31 x 47, 64 x 64 (at S = 64 both passes are copies: the gather alone), 97 x 130 (down-scale), 20 x 24 (up-scale); +-90, 45, 1e-7, 0 with flips
    (reversals alone), 360 (mode 0 from rotate_coeffs) and seeded angles; every flip combination; mode 0 and mode 1 side by side."""
    rng = np.random.default_rng(5)
    r = lambda: float(np.float32(rng.uniform(-90.0, 90.0)))
    return [(7, 5, (45.0, False, False)), (31, 47, (90.0, True, False)), (64, 64, (-90.0, False, True)), (97, 130, (r(), True, True)), (20, 24, (1e-7, False, False)),
            (None, None, None), (31, 47, None), (97, 130, (0.0, False, True)), (64, 64, (r(), True, False)), (20, 24, (r(), False, True)), (7, 5, (360.0, False, False)),
            (64, 64, (90.0, False, False)), (97, 130, (-45.0, False, False)), (31, 47, (r(), True, True))]


_BATCH = {}


def _batch():
    """the arrays and per-slot draws of _pairs(): images first, then the masks (computed once, never changed)"""
    if not _BATCH:
        rng = np.random.default_rng(6)
        pairs = _pairs()
        imgs = [None if h is None else rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w, _ in pairs]
        gts = [None if h is None else rng.integers(0, 256, (h, w, 1), dtype=np.uint8) for h, w, _ in pairs]
        _BATCH.update(arrs=imgs + gts, draws=[d for _, _, d in pairs] * 2, n=len(pairs))
    return _BATCH["arrs"], _BATCH["draws"], _BATCH["n"]


def _run_c_abi(arrs, draws, S, dst, n_rgb, n_mask, plain=False):
    """pn2_input_batch_width_aug (plain: pn2_input_batch_width) and pn2_input_batch_height on guarded buffers.  Returns (rows, aug, taps, tmp bytes, out_rgb,
    out_mask, guards_ok): numpy copies of the scratch arena and the outputs (n_rgb / n_mask samples: one more than the slots fill), and whether every guard and
    every input kept its value."""
    from pn2.capi import call
    from pn2.input import TapArena, batch_table
    dev = _dev()
    taps = TapArena(S)
    shapes = [None if a is None else a.shape for a in arrs]
    rows, src_bytes, tmp_bytes = batch_table(shapes, S, taps, dst=dst, gap=GAP)
    aug = A.aug_rows(shapes, draws)
    src_h = R.pack(arrs, rows, src_bytes, fill=CANARY)
    src = torch.from_numpy(src_h).to(dev)
    tmp = torch.full((tmp_bytes,), CANARY, dtype=torch.uint8, device=dev)
    tap_buf = torch.full((taps.ints + 32,), -1, dtype=torch.int32, device=dev)
    tap_buf[16:16 + taps.ints] = torch.from_numpy(taps.data[:taps.ints].copy()).to(dev)
    aug_h = np.full(64 + aug.nbytes + 64, CANARY, np.uint8)
    aug_h[64:64 + aug.nbytes] = aug.view(np.uint8).reshape(-1)
    aug_d = torch.from_numpy(aug_h).to(dev)
    outs = []
    for n, c in ((n_rgb, 3), (n_mask, 1)):
        buf = torch.full((16 + n * c * S * S + 16,), float(FILL), dtype=torch.float32, device=dev)
        outs.append((buf, buf[16:16 + n * c * S * S]))
    table = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()).to(dev)
    t = _transform(S)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    th, tp = C.c_void_p(rows.ctypes.data), C.c_void_p(tap_buf.data_ptr() + 64)
    if plain:
        call.pn2_input_batch_width(th, _P(table), len(rows), S, _P(src), src_bytes, _P(tmp), tmp_bytes, tp, taps.ints, st)
    else:
        call.pn2_input_batch_width_aug(th, _P(table), C.c_void_p(aug.ctypes.data), C.c_void_p(aug_d.data_ptr() + 64), len(rows), S, _P(src), src_bytes, _P(tmp), tmp_bytes,
                                       tp, taps.ints, st)
    call.pn2_input_batch_height(th, _P(table), len(rows), S, _P(tmp), tmp_bytes, tp, taps.ints, _P(outs[0][1]), n_rgb, _P(outs[1][1]), n_mask, _P(t.mean), _P(t.std), st)
    torch.cuda.synchronize()
    ok = bool(torch.equal(src.cpu(), torch.from_numpy(src_h))) and bool(torch.equal(aug_d.cpu(), torch.from_numpy(aug_h)))          # inputs were only read
    ok &= bool((tap_buf[:16] == -1).all()) and bool((tap_buf[16 + taps.ints:] == -1).all())
    for buf, view in outs:
        ok &= bool((buf[:16] == float(FILL)).all()) and bool((buf[16 + view.numel():] == float(FILL)).all())
    return rows, aug, taps, tmp.cpu().numpy(), outs[0][1].cpu().numpy().reshape(n_rgb, 3, S, S), outs[1][1].cpu().numpy().reshape(n_mask, 1, S, S), ok


def _dst(n):
    return list(range(n)) * 2


@pytest.mark.parametrize("S", [32, 30, 64])
def test_aug_entry_bit_for_bit(S):
    """One ragged batch of images and masks through the C ABI: the whole scratch arena - its canaries between the slots included - equals inputaugref's byte for
    byte, both outputs bit for bit; every sample equals Pillow's rotate, flips and resize followed by ToTensor / Normalize; the empty slots' samples, the samples
    nobody owns and all guards are untouched.  S = 30: rows that do not end on a thread's four pixels (the byte-wise stores); S = 64: the 64 x 64 slots are copied
    by both passes, so their samples are the gather alone."""
    arrs, draws, n = _batch()
    rows, aug, taps, tmp, out_rgb, out_mask, guards = _run_c_abi(arrs, draws, S, _dst(n), n + 1, n + 1)
    assert guards
    modes = [int(g["mode"]) for g in aug]
    assert modes[:n] == modes[n:] == [1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 0, 1, 1, 1]
    src_bytes = int(max(int(r["src"]) + int(r["H"]) * int(r["W"]) * int(r["C"]) for r in rows)) + GAP
    rt, rr, rm = A.run(rows, aug, R.pack(arrs, rows, src_bytes), taps.data, S, len(tmp), n + 1, n + 1, fill=FILL)
    assert np.array_equal(tmp, rt)
    assert np.array_equal(_bits(out_rgb), _bits(rr)) and np.array_equal(_bits(out_mask), _bits(rm))
    assert (out_rgb[5] == FILL).all() and (out_mask[5] == FILL).all() and (out_rgb[-1] == FILL).all() and (out_mask[-1] == FILL).all()
    for i in range(n):
        if arrs[i] is None:
            continue
        assert np.array_equal(_bits(out_rgb[i]), _bits(A.pil_pipeline(arrs[i], draws[i], S, True))), (i, draws[i])
        assert np.array_equal(_bits(out_mask[i]), _bits(A.pil_pipeline(arrs[n + i][:, :, 0], draws[i], S, False))), (i, draws[i])


@pytest.mark.parametrize("S", [32, 30])
def test_mode0_slots_equal_the_plain_entry(S):
    """Every slot in mode 0: the scratch arena and the outputs of pn2_input_batch_width_aug are those of pn2_input_batch_width."""
    arrs, _, n = _batch()
    none = [None] * len(arrs)
    _, aug, _, tmp_a, rgb_a, mask_a, guards_a = _run_c_abi(arrs, none, S, _dst(n), n + 1, n + 1)
    _, _, _, tmp_p, rgb_p, mask_p, guards_p = _run_c_abi(arrs, none, S, _dst(n), n + 1, n + 1, plain=True)
    assert guards_a and guards_p and not aug["mode"].any()
    assert np.array_equal(tmp_a, tmp_p) and np.array_equal(_bits(rgb_a), _bits(rgb_p)) and np.array_equal(_bits(mask_a), _bits(mask_p))
    assert not (tmp_a == CANARY).all()


def _fixture():
    z = np.load(os.path.join(G, "input_aug.npz"))
    return z, sorted({k.split(".")[0] for k in z.files})


def test_batch_with_draws_reproduces_the_fixture():
    """DeviceTransform.batch(images, masks, draws=...) on the sources and decisions of input_aug.npz gives the tensors Pillow made, bit for bit - host arrays and
    device tensors alike; a None among the draws leaves that pair as batch() without draws transforms it."""
    z, names = _fixture()
    by_size = {}
    for n in names:
        by_size.setdefault(z[n + ".x"].shape[-1], []).append(n)
    assert sorted(by_size) == [32, 64]
    for S, group in sorted(by_size.items()):
        t = _transform(S)
        imgs, gts = [z[n + ".img"] for n in group], [z[n + ".gt"] for n in group]
        draws = [(float(z[n + ".draw"][0]), bool(z[n + ".draw"][1]), bool(z[n + ".draw"][2])) for n in group]
        x, g = t.batch(imgs, gts, draws=draws)
        xd, gd = t.batch([torch.from_numpy(a).to(_dev()) for a in imgs], [torch.from_numpy(a).to(_dev()) for a in gts], draws=draws)
        for i, n in enumerate(group):
            assert np.array_equal(_bits(x[i].cpu().numpy()), _bits(z[n + ".x"])) and np.array_equal(_bits(g[i].cpu().numpy()), _bits(z[n + ".g"])), n
        assert torch.equal(x, xd) and torch.equal(g, gd)
        x0, g0 = t.batch(imgs, gts)
        x1, g1 = t.batch(imgs, gts, draws=[None] + draws[1:])
        assert torch.equal(x1[0], x0[0]) and torch.equal(g1[0], g0[0]) and torch.equal(x1[1:], x[1:]) and torch.equal(g1[1:], g[1:])
        with pytest.raises(ValueError, match="draws"):
            t.batch(imgs, gts, draws=draws[1:])


def test_call_pattern_with_and_without_draws(monkeypatch):
    """batch(..., draws=None) calls pn2_input_batch_width and pn2_input_batch_height, once each, and nothing else in the library; a batch of 16 augmented pairs
    calls pn2_input_batch_width_aug once, pn2_input_batch_height once, and nothing else."""
    from pn2 import capi
    from pn2.capi import call
    from pn2.input import DeviceTransform
    t = DeviceTransform(64)
    rng = np.random.default_rng(2)
    sizes = [(41 + 3 * i, 91 - 2 * i) for i in range(16)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    gts = [rng.integers(0, 256, (h, w), dtype=np.uint8) for h, w in sizes]
    np.random.seed(4)
    draws = DeviceTransform.draw(16)
    t.batch(imgs, gts)          # the tap blocks of these sizes (host entries pn2_resize_ksize / pn2_resize_coeffs) are cached now
    counts = {}
    for name in capi.SIGNATURES:
        real = getattr(call, name)
        monkeypatch.setattr(call, name, lambda *a, _r=real, _n=name: (counts.__setitem__(_n, counts.get(_n, 0) + 1), _r(*a))[1], raising=False)
    x0, g0 = t.batch(imgs, gts, draws=None)
    torch.cuda.synchronize()
    assert counts == {"pn2_input_batch_width": 1, "pn2_input_batch_height": 1}, counts
    counts.clear()
    x, g = t.batch(imgs, gts, draws=draws)
    torch.cuda.synchronize()
    assert counts == {"pn2_input_batch_width_aug": 1, "pn2_input_batch_height": 1}, counts
    for i in (0, 7, 15):
        assert np.array_equal(_bits(x[i].cpu().numpy()), _bits(A.pil_pipeline(imgs[i], draws[i], 64, True)))
        assert np.array_equal(_bits(g[i].cpu().numpy()), _bits(A.pil_pipeline(gts[i], draws[i], 64, False)))
    assert not torch.equal(x, x0) and not torch.equal(g, g0)


def _folder(tmp_path, sizes, seed=5):
    from PIL import Image
    rng = np.random.default_rng(seed)
    iroot, groot = str(tmp_path / "images") + "/", str(tmp_path / "masks") + "/"
    os.makedirs(iroot)
    os.makedirs(groot)
    pairs = []
    for k, (h, w) in enumerate(sizes):
        im, gt = rng.integers(0, 256, (h, w, 3), dtype=np.uint8), (rng.random((h, w)) > 0.6).astype(np.uint8) * 255
        Image.fromarray(im, "RGB").save(iroot + f"{k:03d}.png")
        Image.fromarray(gt, "L").save(groot + f"{k:03d}.png")
        pairs.append((im, gt))
    return iroot, groot, pairs


def test_get_loader_augmentation(tmp_path):
    """get_loader(augmentation=True) over four small PNG pairs, numpy's generator seeded: every tensor is the reference pipeline (Pillow rotate, flips, resize,
    ToTensor, Normalize) under the decisions DeviceTransform.draw makes from the same seed, in file order; 'True' and batched=False give the same tensors;
    augmentation=False (and leaving the argument out) gives the tensors without augmentation."""
    from pn2.input import DeviceTransform
    from utils.dataloader import get_loader
    S = 48
    iroot, groot, pairs = _folder(tmp_path, [(40, 60), (48, 35), (31, 31), (50, 45)])
    kw = dict(batchsize=2, trainsize=S, shuffle=False, num_workers=0, pin_memory=False)
    np.random.seed(11)
    draws = DeviceTransform.draw(4)
    want_x = np.stack([A.pil_pipeline(im, d, S, True) for (im, _), d in zip(pairs, draws)])
    want_g = np.stack([A.pil_pipeline(gt, d, S, False) for (_, gt), d in zip(pairs, draws)])
    plain_x = np.stack([A.pil_pipeline(im, None, S, True) for im, _ in pairs])
    plain_g = np.stack([A.pil_pipeline(gt, None, S, False) for _, gt in pairs])
    assert not np.array_equal(want_x, plain_x)
    for args in (dict(augmentation=True), dict(augmentation='True'), dict(augmentation=True, batched=False)):
        loader = get_loader(iroot, groot, **kw, **args)
        assert loader.augmentation is True and len(loader) == 2
        np.random.seed(11)
        got = list(loader)
        x, g = torch.cat([b[0] for b in got]).cpu().numpy(), torch.cat([b[1] for b in got]).cpu().numpy()
        assert got[0][0].is_cuda and x.shape == (4, 3, S, S) and g.shape == (4, 1, S, S)
        assert np.array_equal(_bits(x), _bits(want_x)) and np.array_equal(_bits(g), _bits(want_g)), args
    for args in (dict(), dict(augmentation=False), dict(augmentation='False'), dict(augmentation=False, batched=False)):
        loader = get_loader(iroot, groot, **kw, **args)
        assert loader.augmentation is False
        got = list(loader)
        x, g = torch.cat([b[0] for b in got]).cpu().numpy(), torch.cat([b[1] for b in got]).cpu().numpy()
        assert np.array_equal(_bits(x), _bits(plain_x)) and np.array_equal(_bits(g), _bits(plain_g)), args
