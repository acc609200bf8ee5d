#!/usr/bin/env python3
"""Golden vectors for the augmented input transform of the polyp loaders (multiclass_seg/EMCAD/utils/dataloader.py:24-39): RandomRotation(90),
RandomVerticalFlip, RandomHorizontalFlip, Resize, ToTensor (and Normalize for the image), the image and its mask sharing the random decisions.
torchvision is not installed here; on a PIL image its rotation is Image.rotate(angle, NEAREST, expand=False) with fill 0, its flips are the two transposes
and its Resize is Image.resize(BILINEAR), so the vectors are produced with Pillow itself and the decisions are written down instead of drawn.
Only data is committed:  name.img uint8 [H][W][3], name.gt uint8 [H][W], name.draw float64 (angle, flip_v, flip_h), name.x fp32 [3][S][S], name.g fp32 [1][S][S]."""
import os
import numpy as np
from PIL import Image

rng = np.random.default_rng(11)
mean = np.array([0.485, 0.456, 0.406], np.float32); std = np.array([0.229, 0.224, 0.225], np.float32)
# name, H, W, S, (angle, flip_v, flip_h): a down-scale, an up-scale, a square that Pillow rotates by transposing (both passes are copies), a tiny odd image at
# 45 degrees, flips alone, and an angle so small that only a few pixels move
cases = [("down", 61, 83, 32, (33.7, True, False)), ("up", 20, 24, 32, (-71.25, False, True)), ("square", 64, 64, 64, (90.0, True, True)),
         ("tiny", 7, 5, 32, (45.0, False, False)), ("flips", 31, 47, 32, (0.0, True, True)), ("hair", 40, 40, 32, (1e-7, False, False))]
out = {}
for name, H, W, S, (angle, fv, fh) in cases:
    yy, xx = np.mgrid[0:H, 0:W]
    base = 127 + 100 * np.sin(yy / 7.0)[..., None] * np.cos(xx / 9.0)[..., None] + rng.normal(0, 25, (H, W, 3))
    img = np.clip(base, 0, 255).astype(np.uint8)
    gt = ((yy - H / 2.5) ** 2 + (xx - W / 3.0) ** 2 < (min(H, W) / 2.2) ** 2).astype(np.uint8) * 255
    res = []
    for arr in (img, gt):
        pil = Image.fromarray(arr).rotate(angle, Image.NEAREST, expand=False)
        if fv:
            pil = pil.transpose(Image.FLIP_TOP_BOTTOM)
        if fh:
            pil = pil.transpose(Image.FLIP_LEFT_RIGHT)
        res.append(np.asarray(pil.resize((S, S), Image.BILINEAR)).astype(np.float32) / np.float32(255.0))          # Resize, ToTensor
    out[name + ".img"], out[name + ".gt"] = img, gt
    out[name + ".draw"] = np.array([angle, float(fv), float(fh)], np.float64)
    out[name + ".x"] = np.ascontiguousarray(((res[0] - mean) / std).transpose(2, 0, 1))                             # Normalize (sub then div, fp32)
    out[name + ".g"] = res[1][None]
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "input_aug.npz")
np.savez_compressed(path, **out)
print({k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes")
