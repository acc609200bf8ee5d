"""The ACDC slice pipeline restated per sample on top of tests/zoomref.py: what RandomGenerator of multiclass_seg/EMCAD/utils/dataset_ACDC.py:13-48 collates from slices
of differing, also non-square, shapes, the two zooms of val() (multiclass_seg/MIST/ACDC_train_test.py:58-60,82-83) and medpy's binary Dice (:87) in numpy.
tests/test_raggedref_cpu.py pins it against live scipy; pn2/volinput.py's ragged entry points have to reproduce these arrays exactly.  Also the ragged cases the
tests and tests/golden/acdc_ragged.npz share."""
import numpy as np

import zoomref as Z


def random_generator(images, labels, output_size, draws):
    """RandomGenerator.__call__ + collation of a ragged batch: one zoomref.random_generator call per sample (np.rot90 with odd k swaps a non-square sample's shape
    before the zoom; a sample at the output size after its geometry is not zoomed) -> {'image': float32 [N][1][oh][ow], 'label': int64 [N][oh][ow]}."""
    outs = [Z.random_generator(im[None], lb[None], output_size, [d]) for im, lb, d in zip(images, labels, draws)]
    return {"image": np.concatenate([o["image"] for o in outs]), "label": np.concatenate([o["label"] for o in outs])}


def zoom_ragged(slices, size, order):
    """val()'s way in (order 3) per slice, skipped where the slice has the size already."""
    oh, ow = size
    f = Z.zoom3 if order == 3 else Z.zoom0
    return np.stack([np.array(s) if s.shape == (oh, ow) else f(s, oh, ow) for s in slices])


def unzoom_labels(labels, sizes):
    """val()'s way back: order 0 of every [h][w] label map to its slice's own size, skipped where it has that size."""
    return [np.array(l) if l.shape == tuple(s) else Z.zoom0(l, s[0], s[1]) for l, s in zip(labels, sizes)]


def dice_counts(pred, gt):
    """(|pred != 0 and gt != 0|, |pred != 0|, |gt != 0|): the three integers of medpy.metric.binary.dc."""
    p, g = np.asarray(pred).astype(bool), np.asarray(gt).astype(bool)
    return int(np.count_nonzero(p & g)), int(np.count_nonzero(p)), int(np.count_nonzero(g))


def dc(pred, gt):
    """medpy.metric.binary.dc: 2 |A and B| / (|A| + |B|), 0.0 when both are empty."""
    i, a, b = dice_counts(pred, gt)
    try:
        return 2. * i / float(a + b)
    except ZeroDivisionError:
        return 0.0


# ------------------------------------------------------------------------------------------------ the ragged cases: name -> (output size, [(shape, draw)])
_EDGE_SHAPES = [(31, 63), (32, 64), (33, 65), (65, 63), (63, 31), (64, 32), (65, 33), (63, 65)]          # the 64-lane tile edge and the 32-row transposed tile, both ways
BATCHES = {
    # every k x axis on non-square samples, the loader's extreme angles, axes of length 1 and 2, samples at the output size with and without a geometry and one
    # that reaches it only through the odd-k swap
    "edges": ((28, 40),
              [(s, ("rot_flip", k, a)) for s, (k, a) in zip(_EDGE_SHAPES, [(k, a) for k in range(4) for a in (0, 1)])] +
              [((33, 65), ("rotate", -20)), ((65, 63), ("rotate", -1)), ((31, 63), ("rotate", 0)), ((64, 32), ("rotate", 19))] +
              [((1, 37), None), ((2, 5), ("rot_flip", 1, 1)), ((9, 1), None), ((1, 37), ("rot_flip", 3, 0)), ((7, 2), ("rotate", 7))] +
              [((28, 40), None), ((28, 40), ("rot_flip", 2, 0)), ((28, 40), ("rotate", -7)), ((40, 28), ("rot_flip", 1, 1)), ((40, 28), None), ((40, 28), ("rot_flip", 2, 1))] +
              [((33, 65), None), ((65, 63), None)]),
    # zoomref's zero-edge pair 64 -> 28 (last row at 0), also reached through a swap, next to 48 -> 28 which has no zero edge
    "zero_row": ((28, 28), [((64, 48), None), ((48, 64), ("rot_flip", 3, 0)), ((64, 48), ("rot_flip", 1, 1)), ((28, 28), None), ((64, 64), ("rotate", 19)), ((64, 48), ("rotate", -20))]),
    # 28 -> 48 (last column at 0)
    "zero_col": ((64, 48), [((28, 28), None), ((28, 28), ("rotate", 19)), ((48, 64), ("rot_flip", 3, 1)), ((33, 17), None), ((28, 28), ("rot_flip", 1, 0))]),
    # ACDC-like in-plane sizes at the paper's patch size
    "acdc": ((224, 224), [((154, 224), None), ((216, 256), None)]),
}
ONE = ((28, 40), [((33, 65), ("rot_flip", 1, 0))])          # a batch of one
# val()'s way back: uniform 28 x 40 label maps to these sizes (the second keeps its size)
UNZOOM = ((28, 40), [(65, 63), (28, 40), (1, 37), (40, 28), (64, 48), (2, 5), (33, 65)])


def batch_inputs(name_or_case):
    """(images, labels, draws, size) of a case: float32 / uint8 arrays from zoomref.case_input, the seed the sample's position."""
    size, samples = BATCHES[name_or_case] if isinstance(name_or_case, str) else name_or_case
    pairs = [Z.case_input(s, seed=i) for i, (s, _) in enumerate(samples)]
    return [p[0] for p in pairs], [p[1] for p in pairs], [d for _, d in samples], size


def unzoom_inputs():
    (h, w), sizes = UNZOOM
    return np.stack([Z.case_input((h, w), seed=50 + i)[1] for i in range(len(sizes))]), sizes
