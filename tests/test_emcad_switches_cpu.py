"""CPU checks of the EMCAD decoder switches (concatenation, sequential MSDC, 1x1 LGAG, other kernel-size lists and expansion factors): state_dict against
the reference's manifests, the refusals that stay, the numpy reference of the combine step (tests/msdcref.py) against a torch restatement of the reference's
forward, and the refusal codes of pn2_msdc_combine / pn2_msdc_combine_bwd at the C ABI."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import emcad_swref as S
import msdcref as R

os.environ.setdefault("PN2_NO_PRETRAINED", "1")
F32, BF16 = 0, 1
PTR = C.c_void_p(4096)


# ------------------------------------------------------------------------------------------------ modules
@pytest.mark.parametrize("name", S.NAMES)
def test_switch_state_dict_matches_reference_manifest(name):
    from lib.networks import EMCADNet
    m = EMCADNet(num_classes=S.K, activation="relu6", encoder="pvt_v2_b0", pretrain=False, dual=S.CONFIGS[name][1], **S.switches(name))
    assert [(k, list(v.shape)) for k, v in m.state_dict().items()] == list(S.manifest(name).items())
    S.build(name)                                       # the fixture's weights load strictly


def test_refusals_that_stay():
    from lib.networks import EMCADNet
    mk = lambda **kw: EMCADNet(num_classes=S.K, encoder="pvt_v2_b0", pretrain=False, dual=True, **kw)
    with pytest.raises(NotImplementedError, match="5 x 5"):
        mk(kernel_sizes=[7])
    with pytest.raises(NotImplementedError, match="1 to 4"):
        mk(kernel_sizes=[1, 3, 5, 3, 1])
    with pytest.raises(NotImplementedError):
        mk(activation="gelu")
    with pytest.raises(NotImplementedError, match="1 or 3"):
        mk(lgag_ks=5)
    with pytest.raises(NotImplementedError):
        mk(expansion_factor=1.5)
    with pytest.raises(NotImplementedError):
        EMCADNet(num_classes=S.K, encoder="resnet50", pretrain=False)


# ------------------------------------------------------------------------------------------------ the numpy reference
def _channel_shuffle(x, groups):                        # the reference's channel_shuffle on [M][C] rows
    M, Cc = x.shape
    return x.view(M, groups, Cc // groups).transpose(1, 2).contiguous().view(M, Cc)


def _groups(Cpart, Cw):
    odd = next(g for g in (3, 5, 6, 7, 9, 10, 12) if Cw % g == 0)
    return sorted({g for g in (1, 2, Cpart, Cw, odd) if Cw % g == 0})


@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("mode", ["sum", "cat"])
def test_numpy_reference_matches_torch_restatement(n, mode):
    g = torch.Generator().manual_seed(10 * n + (mode == "cat"))
    M, Cpart = 5, 24
    parts = [torch.randn(M, Cpart, generator=g) for _ in range(n)]
    Cw = n * Cpart if mode == "cat" else Cpart
    for groups in _groups(Cpart, Cw):
        for p in parts:
            p.requires_grad_(True); p.grad = None
        merged = torch.cat(parts, 1) if mode == "cat" else functools.reduce(lambda a, b: a + b, parts)        # ((p0 + p1) + p2) + p3
        want = _channel_shuffle(merged, groups)
        got = R.combine([p.detach().numpy() for p in parts], groups, mode)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.detach().numpy().view(np.uint32)), (groups,)
        dy = torch.randn(M, Cw, generator=g)
        want.backward(dy)
        if mode == "cat":
            gs = R.combine_bwd(dy.numpy(), n, groups)
        else:           # the adjoint of the sum: the sum of one tensor through the inverse shuffle, the gradient of every part
            gs = [R.combine([dy.numpy()], Cw // groups, "sum")] * n
        for p, gi in zip(parts, gs):
            assert np.array_equal(gi.view(np.uint32), p.grad.numpy().view(np.uint32)), (groups,)


def test_numpy_reference_rounds_bf16_to_nearest_even_once():
    v = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.0, 3.3895314e38, 2.0 ** -133], dtype=np.float32)       # ties to even both ways, -0, largest finite, subnormal
    assert R.bf16_bits(v).tolist() == [0x3F80, 0x3F80, 0x3F82, 0x8000, 0x7F7F, 0x0001]
    assert np.array_equal(R.bf16_value(R.bf16_bits(v))[3:].view(np.uint32), v[3:].view(np.uint32))
    a, b, c = (np.full((1, 8), x, dtype=np.float32) for x in (1.0, 2.0 ** -9, 2.0 ** -9))
    # (1 + 2^-9) + 2^-9 = 1 + 2^-8 exactly in fp32: a bf16 tie, rounded to even once at the end
    assert R.bf16_bits(R.combine([a, b, c], 1, "sum", bf16=True)).tolist() == [[0x3F80] * 8]
    acc = R.combine_bwd(np.full((1, 8), 2.0 ** -8, dtype=np.float32), 1, 1, prefill=[np.full((1, 8), 1.0 + 2.0 ** -7, dtype=np.float32)], accumulate=[1], bf16=True)
    assert R.bf16_bits(acc[0]).tolist() == [[0x3F82] * 8]          # 1 + 3 * 2^-8 ties up to even


# ------------------------------------------------------------------------------------------------ refusal codes at the C ABI
def test_msdc_combine_refusals():
    from pn2 import capi
    lib = capi.load()
    for dt, V in ((F32, 4), (BF16, 8)):
        fwd = lambda mode=1, n=3, p=(PTR, PTR, PTR, None), y=PTR, M=512, Cp=64, groups=32, d=dt: lib.pn2_msdc_combine(d, mode, n, p[0], p[1], p[2], p[3], y, M, Cp, groups, None)
        bwd = lambda n=3, dy=PTR, p=(PTR, PTR, PTR, None), M=512, Cp=64, groups=32, d=dt: lib.pn2_msdc_combine_bwd(d, n, dy, p[0], p[1], p[2], p[3], 0, 1, 0, 0, M, Cp, groups, None)
        # -1: a null pointer among the first n parts, y / dy
        for i in range(3):
            hole = tuple(None if k == i else PTR for k in range(3)) + (None,)
            assert fwd(p=hole) == -1 and fwd(mode=0, p=hole) == -1 and bwd(p=hole) == -1, i
        assert fwd(n=4) == -1 and bwd(n=4) == -1                 # the fourth part is required once n = 4
        assert fwd(y=None) == -1 and bwd(dy=None) == -1
        # -2: n, mode, the vector, groups, the built width, M
        full = (PTR,) * 4
        for n in (0, 5, -1):
            assert fwd(n=n, p=full) == -2 and bwd(n=n, p=full) == -2, n
        assert fwd(mode=2) == -2 and fwd(mode=-1) == -2
        for cp in (64 + V // 2, V - 1, 0):
            assert fwd(Cp=cp) == -2 and fwd(mode=0, Cp=cp) == -2 and bwd(Cp=cp) == -2, cp
        assert fwd(groups=5) == -2 and fwd(mode=0, groups=48) == -2 and bwd(groups=5) == -2 and fwd(groups=0) == -2 and bwd(groups=0) == -2
        assert fwd(n=4, p=full, Cp=4096 + V, groups=1) == -2 and bwd(n=4, p=full, Cp=4096 + V, groups=1) == -2          # Cw = 16384 + 4V
        assert fwd(mode=0, n=1, Cp=16384 + V, groups=1) == -2
        for M in (0, -3):
            assert fwd(M=M) == -2 and bwd(M=M) == -2, M
        assert fwd(M=1 << 40, n=4, p=full, Cp=3072, groups=1) == -2           # one pixel per tile: more tiles than a grid holds
        # a valid argument list passes the argument check: only the unknown dtype is left to refuse it
        assert fwd(d=7) == -3 and fwd(mode=0, d=7) == -3 and bwd(d=7) == -3
        assert fwd(d=7, n=4, p=full, Cp=4096, groups=4096) == -3 and bwd(d=7, n=4, p=full, Cp=4096, groups=4096) == -3     # Cw = 16384 is built
        assert fwd(d=7, n=1, mode=0, Cp=8, groups=8) == -3
        # the tile helper: positive where built, -2 where not
        assert lib.pn2_msdc_combine_tile(dt, 16384, 4096) >= 1 and lib.pn2_msdc_combine_tile(dt, 128, 64) > 1
        assert lib.pn2_msdc_combine_tile(dt, 16384 + V, 1) == -2 and lib.pn2_msdc_combine_tile(dt, 64, 5) == -2 and lib.pn2_msdc_combine_tile(dt, 64 + V // 2, 1) == -2
