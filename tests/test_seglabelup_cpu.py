"""CPU tests of the fused label tail: tests/seglabelupref.py (the float32 restatement the GPU tests compare pn2_seg_labels_up with) against torch's own
bilinear interpolation and argmax on inputs where float32 is exact, and the argument checks of the entry point (the library loads without a GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seglabelupref as R


@pytest.mark.parametrize("K", [2, 4, 9, 16])
@pytest.mark.parametrize("shape", [(64, 64), (64, 96)], ids=["64x64", "64x96"])
def test_reference_equals_torch_on_dyadic_inputs(K, shape):
    """argmax(combination of F.interpolate(map, scale_factor=s, mode='bilinear')) of torch on the CPU, N = 3, maps at 1/32 .. 1/4 of the output (s = 32, 16, 8, 4;
    the 2 x 2 and 2 x 3 sources are mostly edge clamping), all three modes with 1, 4 and 8 maps.  The inputs are dyadic (seglabelupref.dyadic_maps): every
    intermediate is exact in float32, so the two agree byte for byte whatever torch contracts or vectorises - and ties between channels occur and are resolved
    towards the lower index by both."""
    OH, OW = shape
    ties = 0.0
    for mode in R.MODES:
        nmaps, scales = R.case(mode)
        maps = R.dyadic_maps(K, K, [(OH // s, OW // s) for s in scales], 3, seed=100 * K + OW + nmaps)
        ups = [F.interpolate(torch.from_numpy(m).permute(0, 3, 1, 2), scale_factor=s, mode="bilinear") for m, s in zip(maps, scales)]
        if mode == "last":
            x = ups[-1]
        elif mode == "sum_fg":
            x = 0.0
            for p in ups:
                x = x + p
        else:
            x = 0.0
            for p, q in zip(ups[:nmaps // 2], ups[nmaps // 2:]):
                x = x + (p - q)
        want = torch.argmax(x, dim=1).numpy().astype(np.uint8)
        for m, s, u in zip(maps, scales, ups):
            assert np.array_equal(R.upsample(m, s), u.permute(0, 2, 3, 1).numpy()), (mode, s)
        got = R.labels(maps, scales, mode, K)
        assert got.shape == (3, OH, OW) and got.dtype == np.uint8
        assert np.array_equal(got, want), mode
        share = R.tie_share(maps, scales, mode, K)
        assert share > 0, mode
        ties = max(ties, share)
        assert len(np.unique(got[1:])) == K, mode          # (every class is predicted somewhere in the samples without the copied channel)
    assert ties >= 0.01


def test_reference_nan_and_tie_rule():
    """The comparison of seg_labels_k: first maximum; a NaN counts as the maximum, the first NaN wins."""
    v = np.array([[1, 3, 3, 2], [np.nan, 5, np.nan, 9], [0, np.nan, 7, np.nan], [2, 2, 2, 2]], np.float32)
    assert R.argmax(v, 4).tolist() == [1, 0, 1, 0]
    assert R.argmax(v, 2).tolist() == [1, 0, 1, 0] and R.argmax(v[:, ::-1].copy(), 3).tolist() == [1, 1, 0, 0]
    assert np.array_equal(R.argmax(v, 4), torch.argmax(torch.from_numpy(v), dim=1).numpy())


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Status codes of pn2_seg_labels_up: -1 for a null pointer or an empty size, -2 outside the built range.  Every call below fails its argument check, which
    comes before the first HIP call: this needs the library but no GPU (the pointers are never dereferenced)."""
    from pn2 import capi
    lib = capi.load()
    one = C.c_void_p(256)

    def maps(ld=16, sizes=None, p=256):
        arr = (capi.SegUpMap * 8)()
        for i, (h, w) in enumerate(sizes or [(2, 2), (4, 4), (8, 8), (16, 16)] * 2):
            arr[i].p, arr[i].ld, arr[i].H, arr[i].W = p, ld, h, w
        return arr
    call = lib.pn2_seg_labels_up
    assert call(None, 4, 1, 3, 9, 64, 64, one, None) == -1
    assert call(maps(), 4, 1, 3, 9, 64, 64, None, None) == -1
    assert call(maps(p=None), 4, 1, 3, 9, 64, 64, one, None) == -1          # a map without a pointer
    assert call(maps(), 4, 1, 0, 9, 64, 64, one, None) == -1                # empty batch
    assert call(maps(), 0, 1, 3, 9, 64, 64, one, None) == -2 and call(maps(), 9, 1, 3, 9, 64, 64, one, None) == -2          # 1..8 maps
    assert call(maps(), 3, 2, 3, 9, 64, 64, one, None) == -2                # odd number of maps for fg - bg
    assert call(maps(), 4, 3, 3, 9, 64, 64, one, None) == -2 and call(maps(), 4, -1, 3, 9, 64, 64, one, None) == -2         # unknown mode
    assert call(maps(), 4, 1, 3, 1, 64, 64, one, None) == -2 and call(maps(), 4, 1, 3, 17, 64, 64, one, None) == -2         # K outside 2..16
    assert call(maps(ld=8), 4, 1, 3, 9, 64, 64, one, None) == -2            # ld < K
    assert call(maps(), 4, 1, 3, 9, 64, 96, one, None) == -2                # 64 / H != 96 / W: two scales
    assert call(maps(), 4, 1, 3, 9, 72, 72, one, None) == -2                # 72 is no multiple of 16
    assert call(maps(sizes=[(64, 32)] * 8), 1, 0, 3, 9, 64, 64, one, None) == -2
    assert call(maps(sizes=[(128, 128)] * 8), 1, 0, 3, 9, 64, 64, one, None) == -2          # a scale below 1
    assert call(maps(sizes=[(0, 0)] * 8), 1, 0, 3, 9, 64, 64, one, None) == -2
    assert call(maps(), 4, 1, 65536, 9, 64, 64, one, None) == -2            # the batch is a grid axis
