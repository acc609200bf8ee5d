"""GPU tests of the ragged-batch input transform: pn2_input_batch_width / pn2_input_batch_height (csrc/pn2_input.hip) through the C ABI with guard bytes around
every arena and output, against the per-image entries (pn2_resize_u8_pass x2 -> pn2_u8_to_tensor, bit for bit), tests/inputbatchref.py and Pillow's stored bytes;
then DeviceTransform.batch, get_loader(batched=...) and test_dataset.load_batch against the per-image paths."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

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


def _slots(S):
    """The sources of the ragged batch under test (3 channels: an image, 1: a mask, None: an empty slot), S standing where the list says 32 - a general case, H == S, W == S, both passes copies, up-scaling with
    ksize 3, down-scaling with a long tap row, one pixel, a mask, an empty slot in the middle, a repeated size, and all-0 / all-255 sources that reach the clip."""
    rng = np.random.default_rng(S)
    u8 = lambda *s: rng.integers(0, 256, s, dtype=np.uint8)
    arrs = [u8(37, 53, 3), u8(S, 80, 3), u8(90, S, 3), u8(S, S, 3), u8(7, 5, 3), u8(200, 150, 3), u8(1, 1, 1), None, u8(53, 37, 1), u8(37, 53, 3),
            np.zeros((11, 13, 3), np.uint8), np.full((13, 11, 3), 255, np.uint8), np.full((6, 9, 1), 255, np.uint8)]
    return arrs


def _per_image(t, a, norm):
    """(scratch image [H][S][C], sample fp32 [C][S][S]) of one source through the per-image entries, called one by one"""
    from pn2.capi import call
    S, dev = t.size, _dev()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    img = torch.from_numpy(a).to(dev)
    H, W, Cc = a.shape
    mid = img
    if W != S:
        xmin, cnt, kk, ks = t._taps(W)
        mid = torch.empty((H, S, Cc), dtype=torch.uint8, device=dev)
        call.pn2_resize_u8_pass(_P(img), _P(mid), H, W, Cc, S, 1, _P(xmin), _P(cnt), _P(kk), ks, st)
    fin = mid
    if H != S:
        xmin, cnt, kk, ks = t._taps(H)
        fin = torch.empty((S, S, Cc), dtype=torch.uint8, device=dev)
        call.pn2_resize_u8_pass(_P(mid), _P(fin), H, S, Cc, S, 0, _P(xmin), _P(cnt), _P(kk), ks, st)
    out = torch.empty((Cc, S, S), dtype=torch.float32, device=dev)
    call.pn2_u8_to_tensor(_P(fin), _P(out), S, S, Cc, _P(t.mean) if norm else None, _P(t.std) if norm else None, st)
    return mid.cpu().numpy(), out.cpu().numpy()


def _run_c_abi(arrs, S, dst, pad, n_rgb, n_mask):
    """The two entries on guarded buffers.  Returns (rows, tmp bytes, out_rgb, out_mask, guards_ok): numpy copies of the scratch arena and of the two outputs
    (n_rgb / n_mask samples: the callers ask for one more than the slots fill, so the last belongs to nobody), and whether every guard kept its value.  pad: guard floats before each
    output - 16 keeps the outputs 16-byte aligned (the wide kernel), 1 does not (the byte kernel)."""
    from pn2.capi import call
    from pn2.input import TapArena, batch_table
    dev = _dev()
    taps = TapArena(S)
    shapes = [None if a is None else a.shape for a in arrs]
    rows, src_bytes, tmp_bytes = batch_table(shapes, S, taps, dst=dst, gap=GAP)
    src_h = R.pack(arrs, rows, src_bytes, fill=CANARY)
    src = torch.from_numpy(src_h).to(dev)
    tmp = torch.full((tmp_bytes,), CANARY, dtype=torch.uint8, device=dev)
    tap_buf = torch.full((taps.ints + 32,), -1, dtype=torch.int32, device=dev)
    tap_buf[16:16 + taps.ints] = torch.from_numpy(taps.data[:taps.ints].copy()).to(dev)
    outs = []
    for n, c in ((n_rgb, 3), (n_mask, 1)):
        buf = torch.full((pad + n * c * S * S + 16,), float(FILL), dtype=torch.float32, device=dev)
        outs.append((buf, buf[pad:pad + n * c * S * S]))
    table = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()).to(dev)
    t = _transform(S)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    th, tp = C.c_void_p(rows.ctypes.data), C.c_void_p(tap_buf.data_ptr() + 64)
    call.pn2_input_batch_width(th, _P(table), len(rows), S, _P(src), src_bytes, _P(tmp), tmp_bytes, tp, taps.ints, st)
    call.pn2_input_batch_height(th, _P(table), len(rows), S, _P(tmp), tmp_bytes, tp, taps.ints, _P(outs[0][1]), n_rgb, _P(outs[1][1]), n_mask, _P(t.mean), _P(t.std), st)
    torch.cuda.synchronize()
    ok = bool(torch.equal(src.cpu(), torch.from_numpy(src_h)))                                  # the source arena, canaries included, was only read
    ok &= bool((tap_buf[:16] == -1).all()) and bool((tap_buf[16 + taps.ints:] == -1).all())
    for buf, view in outs:
        ok &= bool((buf[:pad] == float(FILL)).all()) and bool((buf[pad + view.numel():] == float(FILL)).all())
    return rows, taps, tmp.cpu().numpy(), outs[0][1].cpu().numpy().reshape(n_rgb, 3, S, S), outs[1][1].cpu().numpy().reshape(n_mask, 1, S, S), ok


_T = {}


def _transform(S):
    from pn2.input import DeviceTransform
    if S not in _T:
        _T[S] = DeviceTransform(S)
    return _T[S]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("S,pad", [(32, 16), (44, 16), (32, 1), (30, 16)])
def test_batch_entries_bit_for_bit(S, pad):
    """One ragged batch through the C ABI: every sample's fp32 bits equal the per-image entries' and inputbatchref's, every scratch image its bytes; the empty
    slot's sample, the sample nobody owns and all guards are untouched; the batch in another slot order gives each image the same bits.  (32, 1): outputs that are
    only 4-byte aligned; S = 30: rows that do not end on a thread's four pixels - both take the byte-wise kernel."""
    arrs = _slots(S)
    is_img = [a is None or a.shape[2] == 3 for a in arrs]
    dst, seen = [], {True: 0, False: 0}
    for im in is_img:
        dst.append(seen[im])
        seen[im] += 1
    rows, taps, tmp, out_rgb, out_mask, guards = _run_c_abi(arrs, S, dst, pad, seen[True] + 1, seen[False] + 1)
    assert guards
    # --- inputbatchref: the whole scratch arena (its canaries between the slots included) and both outputs (the untouched samples included)
    src_bytes = int(max(int(r["src"]) + int(r["H"]) * int(r["W"]) * int(r["C"]) for r in rows)) + GAP
    rt, rr, rm = R.run(rows, R.pack(arrs, rows, src_bytes), taps.data, S, len(tmp), out_rgb.shape[0], out_mask.shape[0], fill=FILL)
    assert np.array_equal(tmp, rt)
    assert np.array_equal(_bits(out_rgb), _bits(rr)) and np.array_equal(_bits(out_mask), _bits(rm))
    assert (out_rgb[dst[7]] == FILL).all() and (out_rgb[-1] == FILL).all() and (out_mask[-1] == FILL).all()          # slot 7 is the empty one
    # --- the per-image entries
    t = _transform(S)
    for i, a in enumerate(arrs):
        if a is None:
            continue
        mid, ref = _per_image(t, a, norm=is_img[i])
        r = rows[i]
        got_mid = tmp[int(r["tmp"]):int(r["tmp"]) + mid.size].reshape(mid.shape)
        assert np.array_equal(got_mid, mid), i
        got = (out_rgb if is_img[i] else out_mask)[dst[i]]
        assert np.array_equal(_bits(got), _bits(ref)), (i, a.shape)
    assert float(out_rgb[dst[10]].max()) < 0 and float(out_mask[dst[12]].min()) == 1.0          # all-0 image (normalised), all-255 mask
    # --- another slot order, the same destinations
    perm = [12, 3, 7, 0, 9, 5, 1, 11, 2, 8, 4, 10, 6]
    _, _, _, out_rgb2, out_mask2, guards2 = _run_c_abi([arrs[p] for p in perm], S, [dst[p] for p in perm], pad, seen[True] + 1, seen[False] + 1)
    assert guards2 and np.array_equal(_bits(out_rgb), _bits(out_rgb2)) and np.array_equal(_bits(out_mask), _bits(out_mask2))


def test_batch_entries_pillow_fixtures():
    """The images and masks of input_pipeline.npz, one batch per output size (352 among them): the samples are ToTensor / Normalize of the bytes Pillow stored."""
    z = np.load(os.path.join(G, "input_pipeline.npz"))
    by_size = {}
    for n in sorted({k.split(".")[0] for k in z.files}):
        by_size.setdefault(z[n + ".resized"].shape[0], []).append(n)
    assert 352 in by_size
    for S, group in sorted(by_size.items()):
        arrs = [z[n + ".in"] if z[n + ".in"].ndim == 3 else z[n + ".in"][:, :, None] for n in group]
        dst, seen = [], {3: 0, 1: 0}
        for a in arrs:
            dst.append(seen[a.shape[2]])
            seen[a.shape[2]] += 1
        _, _, _, out_rgb, out_mask, guards = _run_c_abi(arrs, S, dst, 16, seen[3] + 1, seen[1] + 1)
        assert guards
        for n, a, d in zip(group, arrs, dst):
            img = a.shape[2] == 3
            got = (out_rgb if img else out_mask)[d]
            assert np.array_equal(_bits(got), _bits(R.to_tensor(z[n + ".resized"].reshape(S, S, -1), img))), n
            if n + ".tensor" in z.files:
                assert np.array_equal(_bits(got), _bits(z[n + ".tensor"])), n


def _host_batch(seed=1):
    rng = np.random.default_rng(seed)
    sizes = [(70, 91), (96, 96), (211, 257), (96, 40), (33, 96), (70, 91)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    gts = [rng.integers(0, 2, (h, w), dtype=np.uint8) * 255 for h, w in sizes]
    return imgs, gts


def test_device_transform_batch_equals_call():
    """batch() == __call__ (torch.equal on x and g) for numpy arrays, CPU tensors and device tensors; a second batch of known sizes uploads no tap block; an empty
    slot keeps its sample; images alone return x alone."""
    from pn2.input import DeviceTransform
    dev = _dev()
    imgs, gts = _host_batch()
    t = DeviceTransform(96)
    x0, g0 = t([torch.from_numpy(a).to(dev) for a in imgs], [torch.from_numpy(a).to(dev) for a in gts])
    x1, g1 = t.batch(imgs, gts)
    assert x1.shape == (6, 3, 96, 96) and g1.shape == (6, 1, 96, 96) and torch.equal(x1, x0) and torch.equal(g1, g0)
    assert t.tap_uploads == 1 and sorted(t.taps.blocks) == [33, 40, 70, 91, 211, 257]
    ints = t.taps.ints
    x2, g2 = t.batch([torch.from_numpy(a) for a in imgs], [torch.from_numpy(a) for a in gts])                      # CPU tensors
    x3, g3 = t.batch([torch.from_numpy(a).to(dev) for a in imgs], [torch.from_numpy(a).to(dev) for a in gts])      # device tensors
    x4, g4 = t.batch([imgs[0], torch.from_numpy(imgs[1]).to(dev)] + imgs[2:], gts)                                  # mixed
    for x, g in ((x2, g2), (x3, g3), (x4, g4)):
        assert torch.equal(x, x0) and torch.equal(g, g0)
    assert t.tap_uploads == 1 and t.taps.ints == ints          # known sizes: only the table went up
    x5 = t.batch(imgs[:2] + [rng_image(50, 61)])
    assert isinstance(x5, torch.Tensor) and torch.equal(x5[:2], x0[:2]) and t.tap_uploads == 2 and sorted(t.taps.blocks) == [33, 40, 50, 61, 70, 91, 211, 257]
    xo, go = torch.full_like(x0, 3.0), torch.full_like(g0, 3.0)
    xr, gr = t.batch([imgs[0], None] + imgs[2:], gts[:4] + [None, gts[5]], out=(xo, go))
    assert xr is xo and gr is go and bool((xo[1] == 3.0).all()) and bool((go[4] == 3.0).all())
    keep = [0, 2, 3, 4, 5]
    assert torch.equal(xo[keep], x0[keep]) and torch.equal(go[[0, 1, 2, 3, 5]], g0[[0, 1, 2, 3, 5]])
    e = t.batch([])
    assert e.shape == (0, 3, 96, 96)
    with pytest.raises(RuntimeError, match="RGB"):
        t.batch([gts[0]])
    with pytest.raises(RuntimeError, match="uint8"):
        t.batch([imgs[0].astype(np.float32)])


def rng_image(h, w):
    return np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_batch_of_16_with_masks_is_two_launches(monkeypatch):
    """One batch(...) call of 16 images with masks: one call of each batch entry (one launch each, csrc/pn2_input.hip) and of nothing else in the library."""
    from pn2 import capi
    from pn2.capi import call
    from pn2.input import DeviceTransform
    t = DeviceTransform(64)
    rng = np.random.default_rng(2)
    sizes = [(41 + 3 * i, 91 - 2 * i) for i in range(16)]          # no axis of length 64: the per-image path runs both passes
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    gts = [rng.integers(0, 256, (h, w), dtype=np.uint8) for h, w in sizes]
    t.batch(imgs, gts)          # the tap blocks of these sizes (host entries pn2_resize_ksize / pn2_resize_coeffs) are cached now
    counts = {}
    for name in capi.SIGNATURES:
        real = getattr(call, name)
        monkeypatch.setattr(call, name, lambda *a, _r=real, _n=name: (counts.__setitem__(_n, counts.get(_n, 0) + 1), _r(*a))[1], raising=False)
    x, g = t.batch(imgs, gts)
    torch.cuda.synchronize()
    assert counts == {"pn2_input_batch_width": 1, "pn2_input_batch_height": 1}, counts
    x0, g0 = t([torch.from_numpy(a).to(_dev()) for a in imgs], [torch.from_numpy(a).to(_dev()) for a in gts])
    assert torch.equal(x, x0) and torch.equal(g, g0)
    assert counts["pn2_resize_u8_pass"] == 64 and counts["pn2_u8_to_tensor"] == 32          # what the per-image path issues for the same batch


def _folder(tmp_path, sizes, seed=5):
    from PIL import Image
    rng = np.random.default_rng(seed)
    iroot, groot = str(tmp_path / "images") + "/", str(tmp_path / "masks") + "/"
    os.makedirs(iroot)
    os.makedirs(groot)
    for k, (h, w) in enumerate(sizes):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(iroot + f"{k:03d}.png")
        Image.fromarray((rng.random((h, w)) > 0.6).astype(np.uint8) * 255, "L").save(groot + f"{k:03d}.png")
    return iroot, groot


def test_get_loader_batched_equals_per_image(tmp_path):
    from utils.dataloader import get_loader
    iroot, groot = _folder(tmp_path, [(80, 120), (96, 70), (61, 61), (100, 90), (96, 96)])
    kw = dict(batchsize=2, trainsize=96, shuffle=False, num_workers=0, pin_memory=False)
    a, b, c = get_loader(iroot, groot, **kw), get_loader(iroot, groot, batched=True, **kw), get_loader(iroot, groot, batched=False, **kw)
    assert a.batched is True and c.batched is False and len(b) == len(c) == 3
    n = 0
    for (xa, ga), (xb, gb), (xc, gc) in zip(a, b, c):
        assert xb.is_cuda and xb.shape == xc.shape and xb.shape[1:] == (3, 96, 96) and gb.shape[1:] == (1, 96, 96)
        assert torch.equal(xb, xc) and torch.equal(gb, gc) and torch.equal(xa, xc) and torch.equal(ga, gc)
        n += xb.shape[0]
    assert n == 5


def test_load_batch_equals_load_data(tmp_path):
    from utils.dataloader import test_dataset
    iroot, groot = _folder(tmp_path, [(80, 120), (64, 70), (61, 61), (100, 90), (64, 64)], seed=6)
    one, many = test_dataset(iroot, groot, 64), test_dataset(iroot, groot, 64)
    singles = [one.load_data() for _ in range(5)]
    got = []
    for k, m in ((2, 2), (2, 2), (2, 1), (2, 0)):
        images, gts, names = many.load_batch(k)
        assert images.shape == (m, 3, 64, 64) and len(gts) == len(names) == m
        got += [(images[j:j + 1], gts[j], names[j]) for j in range(m)]
    assert many.index == 5 and len(got) == 5
    for (xs, gs, ns), (xb, gb, nb) in zip(singles, got):
        assert ns == nb and torch.equal(xs, xb) and gs.size == gb.size and gs.mode == gb.mode == "L" and np.array_equal(np.asarray(gs), np.asarray(gb))


def test_test_with_eval_uses_load_batch(tmp_path):
    """Predictor.test_with_eval over a test_dataset (load_batch) returns what it returns over the list of the same set's load_data() triples."""
    import pn2
    from pn2.infer import Predictor
    from lib.pranet import PraNet_V2
    from oracle import weights as W
    from utils.dataloader import test_dataset
    iroot, groot = _folder(tmp_path, [(80, 120), (64, 70), (61, 61), (100, 90), (64, 64)], seed=7)
    was = pn2.get_compute_dtype()
    pn2.set_compute_dtype("fp32")
    try:
        model = PraNet_V2(num_class=1)
        model.load_state_dict(W.make_state_dict(W.manifest_pranet_v2(1), seed=0, bn3_gamma=0.05), strict=True)
        pred = Predictor(model.to(_dev()).eval())
        opt = {"metrics": ["meanDic", "meanIoU", "wFm", "Sm", "meanEm", "mae"]}
        one = test_dataset(iroot, groot, 64)
        items = [one.load_data() for _ in range(5)]
        ref, ref_mean = pred.test_with_eval(items, opt, batch_size=2)
        ds = test_dataset(iroot, groot, 64)
        res, mean = pred.test_with_eval(ds, opt, batch_size=2)
        assert ds.index == 5 and res.shape == (5, 6)
        assert np.array_equal(res, ref, equal_nan=True) and np.array_equal(mean, ref_mean, equal_nan=True)
    finally:
        pn2.set_compute_dtype(was)
