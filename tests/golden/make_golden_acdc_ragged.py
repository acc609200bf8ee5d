"""Writes tests/golden/acdc_ragged.npz: numpy's and scipy.ndimage's own outputs on the ragged cases of tests/raggedref.py, so that the GPU tests of the ragged
entry points of pn2/volinput.py compare with scipy without importing it.  Per batch "<name>": image float32 [N][oh][ow] and label uint8 [N][oh][ow] - per sample
np.flip(np.rot90(a, k), axis) or ndimage.rotate(a, angle, order=0, reshape=False) or nothing, then ndimage.zoom of order 3 / order 0 unless the sample has the output
size by then.  "unzoom/<i>": ndimage.zoom(order=0) of label map i to its own size.  The inputs are raggedref.batch_inputs / unzoom_inputs (numpy's PCG64) and are not
stored.  Run: python tests/golden/make_golden_acdc_ragged.py (needs scipy)."""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import raggedref as R  # noqa: E402


def sample(im, lb, draw, size):
    if draw is not None and draw[0] == "rot_flip":
        im, lb = np.flip(np.rot90(im, draw[1]), axis=draw[2]).copy(), np.flip(np.rot90(lb, draw[1]), axis=draw[2]).copy()
    elif draw is not None:
        im, lb = ndimage.rotate(im, draw[1], order=0, reshape=False), ndimage.rotate(lb, draw[1], order=0, reshape=False)
    x, y = im.shape
    if (x, y) != tuple(size):
        im, lb = ndimage.zoom(im, (size[0] / x, size[1] / y), order=3), ndimage.zoom(lb, (size[0] / x, size[1] / y), order=0)
    return im.astype(np.float32), lb.astype(np.uint8)


out = {}
for name in R.BATCHES:
    images, labels, draws, size = R.batch_inputs(name)
    pairs = [sample(im, lb, d, size) for im, lb, d in zip(images, labels, draws)]
    out[name + "/image"], out[name + "/label"] = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
maps, sizes = R.unzoom_inputs()
for i, (m, s) in enumerate(zip(maps, sizes)):
    out[f"unzoom/{i}"] = m.copy() if m.shape == tuple(s) else ndimage.zoom(m, (s[0] / m.shape[0], s[1] / m.shape[1]), order=0)
path = os.path.join(HERE, "acdc_ragged.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes,", len(out), "arrays")
