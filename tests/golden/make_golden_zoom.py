"""Writes tests/golden/synapse_zoom.npz: scipy.ndimage's own outputs on the inputs of tests/zoomref.py:case_input, so that the GPU tests of pn2/volinput.py
compare with scipy without importing it.  Per zoom case "<H>x<W>_<oh>x<ow>": img, lab (the inputs), out3 = zoom(img, order=3), out0 = zoom(lab, order=0).
The 512² -> 224² case stores the outputs only (its input is case_input((512, 512))); 224² -> 512² is left to zoomref, which tests/test_zoomref_cpu.py pins
against scipy at that shape.  Per rotate shape "rot<H>x<W>": u8 [40][H][W] = rotate(lab, angle, order=0, reshape=False) for angle in range(-20, 20), and
f32 likewise for the smaller shape.  Run: python tests/golden/make_golden_zoom.py (needs scipy)."""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zoomref as Z  # noqa: E402

out = {}
for src, dst in Z.SHAPES:
    if src == (224, 224):
        continue
    img, lab = Z.case_input(src)
    key = Z.case_key(src, dst)
    fac = (dst[0] / src[0], dst[1] / src[1])
    if src != (512, 512):
        out[key + "/img"], out[key + "/lab"] = img, lab
    out[key + "/out3"], out[key + "/out0"] = ndimage.zoom(img, fac, order=3), ndimage.zoom(lab, fac, order=0)
for shape in Z.ROTATE_SHAPES:
    img, lab = Z.case_input(shape, seed=1)
    key = f"rot{shape[0]}x{shape[1]}"
    out[key + "/u8"] = np.stack([ndimage.rotate(lab, a, order=0, reshape=False) for a in Z.ANGLES])
    if shape == Z.ROTATE_SHAPES[0]:
        out[key + "/f32"] = np.stack([ndimage.rotate(img, a, order=0, reshape=False) for a in Z.ANGLES])
path = os.path.join(HERE, "synapse_zoom.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes,", len(out), "arrays")
