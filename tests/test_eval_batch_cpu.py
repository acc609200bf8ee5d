"""CPU tests of the batched test-set evaluation (pn2/evaltail.py): the pure host finish metrics_from_counts, fed with counts that numpy and the oracle compute
(what pn2_eval_hist / pn2_eval_region_sums / pn2_eval_wfm count on the device), against the reference's eval_for_testAllInOne values stored in
tests/golden/eval_full.npz; and the builder of the ragged batch's device table."""
import os
import warnings

import numpy as np
import pytest

from oracle import pranet_oracle as O

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["meanDic", "meanIoU", "wFm", "Sm", "meanEm", "mae"]
TAGS = ("blob", "zero_pred", "exact", "full", "two", "rand352")


def counts_numpy(pred_u8, gt):
    """(h_all, h_gt, out25, (s_fg, s_bg)) of one image as include/pn2.h defines them, with numpy and the oracle's restatement of scipy."""
    g = np.asarray(gt) > 0.5
    H, W = g.shape
    h_all = np.bincount(pred_u8.reshape(-1), minlength=256).astype(np.int64)
    h_gt = np.bincount(pred_u8[g], minlength=256).astype(np.int64)
    out25 = [0] * 25
    rr, cc = np.nonzero(g)
    out25[0], out25[1], out25[2] = int(rr.sum()), int(cc.sum()), int(g.sum())
    X, Y = (int(np.rint(rr.sum() / g.sum())), int(np.rint(cc.sum() / g.sum()))) if g.sum() else (H // 2, W // 2)
    k = pred_u8.astype(np.int64)
    for q in range(4):
        a = slice(X, None) if q & 1 else slice(None, X)
        b = slice(Y, None) if q & 2 else slice(None, Y)
        kq, gq = k[a, b], g[a, b].astype(np.int64)
        out25[3 + 5 * q: 8 + 5 * q] = [int(kq.size), int(kq.sum()), int((kq * kq).sum()), int(gq.sum()), int((kq * gq).sum())]
    out25[23], out25[24] = X, Y
    sums = None
    if g.any():
        from pn2.evaltail import gauss7
        pred = pred_u8.astype(np.float64) / 255
        gd = g.astype(np.float64)
        Eabs = np.abs(pred - gd)
        dst, ri, rj = O.edt_nearest(gd)
        Et = Eabs.copy()
        Et[~g] = Eabs[ri[~g], rj[~g]]
        EA = O.conv_nearest(Et, gauss7())
        mn = Eabs.copy()
        sel = g & (EA < Eabs)
        mn[sel] = EA[sel]
        Bw = np.ones_like(gd)
        Bw[~g] = 2.0 - 1 * np.exp(np.log(1 - 0.5) / 5 * dst[~g])
        Ew = mn * Bw
        sums = (float(Ew[g].sum()), float(Ew[~g].sum()))
    return h_all, h_gt, out25, sums


@pytest.mark.parametrize("tag", TAGS)
def test_metrics_from_counts_vs_reference(tag):
    """All six metrics within 1e-9 * max(1, |ref|) of the reference's stored values (the bound of test_full_eval_metrics_vs_reference_eval_for_testAllInOne), the
    EnhancedMeasure curve within 1e-12; no torch tensor and no GPU in the function under test."""
    from pn2.evaltail import metrics_from_counts
    z = np.load(os.path.join(G, "eval_full.npz"))
    pred, gt = z[tag + "_pred"], z[tag + "_gt"]
    h_all, h_gt, out25, sums = counts_numpy(pred, gt)
    r = metrics_from_counts(h_all, h_gt, out25, sums, *pred.shape)
    for k, ref in zip(NAMES, z[tag + "_vals"]):
        assert abs(r[k] - float(ref)) <= 1e-9 * max(1.0, abs(float(ref))), (tag, k, r[k], float(ref))
    assert np.abs(r["E"] - z[tag + "_E"]).max() <= 1e-12, tag
    # the threshold sweep alone, and the keys a caller did not supply counts for
    t = metrics_from_counts(h_all, h_gt, full=False)
    assert sorted(t) == ["curves", "mae", "meanDic", "meanFm", "meanIoU", "meanSen", "meanSpe"] and t["meanDic"] == r["meanDic"] and t["mae"] == r["mae"]
    part = metrics_from_counts(h_all, h_gt)
    assert part["meanEm"] == r["meanEm"] and ("wFm" in part) == (h_gt.sum() == 0) and ("Sm" in part) == (h_gt.sum() in (0, h_all.sum()))
    with pytest.raises(ValueError):
        metrics_from_counts(h_all, h_gt, out25, sums, pred.shape[0] + 1, pred.shape[1])


def test_metrics_from_counts_without_foreground():
    from pn2.evaltail import metrics_from_counts
    z = np.load(os.path.join(G, "eval_full.npz"))
    pred = z["blob_pred"]
    h_all, h_gt, out25, sums = counts_numpy(pred, np.zeros_like(z["blob_gt"]))
    assert sums is None
    r = metrics_from_counts(h_all, h_gt, out25, None, *pred.shape)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        o = O.full_metrics(pred, np.zeros_like(z["blob_gt"]))
    assert abs(r["Sm"] - o["Sm"]) < 1e-12 and abs(r["meanEm"] - o["meanEm"]) < 1e-12 and np.isnan(r["wFm"])


def test_ragged_table():
    from pn2.evaltail import ragged_table, ROW
    assert ROW.itemsize == 24 and [ROW.fields[n][1] for n in ("H", "W", "off", "rh", "rw")] == [0, 4, 8, 16, 20]
    shapes = [(17, 23), (40, 31), None, (24, 24), (1, 1), (7, 50)]
    rows, total = ragged_table(shapes, 24, 16, slots=8)
    assert len(rows) == 8 and total == 17 * 23 + 40 * 31 + 24 * 24 + 1 + 7 * 50
    off = 0
    for b, s in enumerate(shapes + [None, None]):
        if s is None:
            assert rows[b]["H"] == 0 and rows[b]["W"] == 0          # an empty slot
            continue
        assert (rows[b]["H"], rows[b]["W"], rows[b]["off"]) == (s[0], s[1], off)
        # the double quotient rounded ONCE to fp32 (not the quotient of two fp32 numbers, not 1 / scale)
        assert rows[b]["rh"] == np.float32(24 / s[0]) and rows[b]["rw"] == np.float32(16 / s[1]) and rows[b]["rh"].dtype == np.float32
        off += s[0] * s[1]
    assert rows[0]["off"] == 0 and rows[1]["off"] % 2 == 1          # offsets are aligned to nothing
    # gaps for canaries: before every image and after the last
    rows, total = ragged_table([(3, 5), None, (2, 2)], 8, 8, gap=3)
    assert [int(r["off"]) for r in rows] == [3, 0, 21] and total == 28
    with pytest.raises(ValueError):
        ragged_table([(3, 5)] * 3, 8, 8, slots=2)
