"""GPU tests of csrc/pn2_resnet.hip at the C ABI - the strided gather and its adjoint move bits, so they must equal torch slicing / scatter bit for bit - and of
Engine.strided_pointwise against the generic stride-2 conv_bn_act on the same nn.Conv2d."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
os.environ.setdefault("PN2_NO_PRETRAINED", "1")

dev = "cuda"
P_ = lambda t: C.c_void_p(t.data_ptr())
SHAPES = [(1, 1, 1), (2, 2, 2), (2, 7, 5), (1, 8, 8), (3, 9, 16)]          # a single pixel, odd extents, a row tail that does not fill a wave
WIDTHS = [8, 24, 256]
CANARY = 3                                                               # rows of `ld` elements in front of and behind every buffer


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()
    yield
    pn2.set_compute_dtype("bf16")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy()


class _Buf:
    """[CANARY + M + CANARY][ld] of random values; .body = the M rows a kernel may touch (their columns >= C it may not)."""

    def __init__(self, shape, ld, tdt, gen):
        self.shape, self.ld, self.M = shape, ld, shape[0] * shape[1] * shape[2]
        self.full = torch.randn(self.M + 2 * CANARY, ld, generator=gen).to(tdt).to(dev)
        self.before = self.full.clone()
        self.body = self.full[CANARY:CANARY + self.M]

    def view(self, t=None):
        t = self.body if t is None else t[CANARY:CANARY + self.M]
        return t.view(*self.shape, self.ld)

    def untouched_outside(self, Cc):
        """the canary rows and the columns past C hold what they held"""
        a, b = _bits(self.full), _bits(self.before)
        return (np.array_equal(a[:CANARY], b[:CANARY]) and np.array_equal(a[CANARY + self.M:], b[CANARY + self.M:])
                and np.array_equal(a[CANARY:CANARY + self.M, Cc:], b[CANARY:CANARY + self.M, Cc:]))


@pytest.mark.parametrize("dtn", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_subsample_c_abi_bit_exact(dtn, shape):
    from pn2 import capi, F32, BF16
    lib = capi.load()
    dt, tdt = (F32, torch.float32) if dtn == "fp32" else (BF16, torch.bfloat16)
    N, H, W = shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator().manual_seed(N * 10000 + H * 100 + W)
    for Cc in WIDTHS:
        for ld in (Cc, Cc + 16):
            # ---- forward
            x, y = _Buf((N, H, W), ld, tdt, gen), _Buf((N, OH, OW), ld, tdt, gen)
            want = x.view()[:, ::2, ::2, :Cc]
            runs = []
            for _ in range(2):
                y.full.copy_(y.before)
                assert lib.pn2_subsample_fwd(dt, P_(x.body), ld, P_(y.body), ld, N, H, W, Cc, 2, st) == 0
                torch.cuda.synchronize()
                runs.append(_bits(y.view()[..., :Cc]))
            assert np.array_equal(runs[0], _bits(want)), (Cc, ld)
            assert np.array_equal(runs[0], runs[1])
            assert y.untouched_outside(Cc) and x.untouched_outside(0), (Cc, ld)
            # ---- backward, both orders of arrival
            for accum in (0, 1):
                dy, dx = _Buf((N, OH, OW), ld, tdt, gen), _Buf((N, H, W), ld, tdt, gen)
                prior = dx.view(dx.before)[..., :Cc]
                want = prior.clone() if accum else torch.zeros_like(prior)
                want[:, ::2, ::2] = (prior[:, ::2, ::2] + dy.view()[..., :Cc]) if accum else dy.view()[..., :Cc]
                runs = []
                for _ in range(2):
                    dx.full.copy_(dx.before)
                    assert lib.pn2_subsample_bwd(dt, P_(dy.body), ld, P_(dx.body), ld, N, H, W, Cc, 2, accum, st) == 0
                    torch.cuda.synchronize()
                    runs.append(_bits(dx.view()[..., :Cc]))
                assert np.array_equal(runs[0], _bits(want)), (Cc, ld, accum)
                assert np.array_equal(runs[0], runs[1])
                if accum:          # the pixels between the strided ones keep the pattern written beforehand
                    keep = torch.ones(H, W, dtype=torch.bool); keep[::2, ::2] = False
                    assert np.array_equal(_bits(dx.view()[:, keep][..., :Cc]), _bits(prior[:, keep]))
                assert dx.untouched_outside(Cc) and dy.untouched_outside(0), (Cc, ld, accum)


@pytest.mark.parametrize("dtn", ["bf16", "fp32"])
def test_subsample_stride1_is_a_copy(dtn):
    from pn2 import capi, F32, BF16
    lib = capi.load()
    dt, tdt = (F32, torch.float32) if dtn == "fp32" else (BF16, torch.bfloat16)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = torch.randn(2, 5, 3, 24).to(tdt).to(dev)
    y = torch.zeros_like(x)
    assert lib.pn2_subsample_fwd(dt, P_(x), 24, P_(y), 24, 2, 5, 3, 24, 1, st) == 0
    assert lib.pn2_subsample_bwd(dt, P_(x), 24, P_(y), 24, 2, 5, 3, 24, 1, 1, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(y), _bits(x + x))


def test_refused_calls_write_nothing():
    from pn2 import capi, F32, BF16
    lib = capi.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    src = torch.ones(1 << 14, device=dev)
    dst = torch.zeros(1 << 14, device=dev)
    s, d, nul = P_(src), P_(dst), C.c_void_p(0)
    calls = [(lib.pn2_subsample_fwd, lambda **k: (k.get("dt", F32), k.get("a", s), k.get("ld", 16), k.get("b", d), k.get("ld", 16), 2, 8, 8, k.get("C", 16), k.get("stride", 2), st)),
             (lib.pn2_subsample_bwd, lambda **k: (k.get("dt", F32), k.get("a", s), k.get("ld", 16), k.get("b", d), k.get("ld", 16), 2, 8, 8, k.get("C", 16), k.get("stride", 2), 0, st))]
    for fn, args in calls:
        assert fn(*args(a=nul)) == -1
        assert fn(*args(dt=5)) == -3
        for bad in (dict(stride=0), dict(stride=3), dict(C=6), dict(dt=BF16, C=12), dict(ld=18), dict(b=C.c_void_p(dst.data_ptr() + 4))):
            assert fn(*args(**bad)) == -2, bad
    torch.cuda.synchronize()
    assert float(dst.abs().max()) == 0.0


def test_strided_pointwise_matches_generic_strided_conv():
    """Engine.strided_pointwise (gather + stride-1 pointwise path) against conv_bn_act on the SAME nn.Conv2d(64, 128, 1, stride=2) - the implicit GEMM with the stride in its
    index math, the path the parent commit takes - in fp32 train mode, 2 x 8 x 8 x 64 -> 2 x 4 x 4 x 128: forward, dx, dW and the BatchNorm parameter gradients.

    Bound.  Both paths evaluate the same expressions on the same operands; what may differ is the order of their fp32 sums.  Reordering a sum of n terms moves it by at
    most 2 (n - 1) u sum|terms| (u = 2^-24).  The sums: the contraction over Cin = 64, the BatchNorm batch sums over M = 32 pixels (mean, variance; backward: the two
    reduction sums), the weight gradient over M = 32, the data gradient over Cout = 128 - at most S = 4 of them chained between the inputs and any result, none longer
    than L = 128.  With sum|terms| <= L max|term| and operands of O(1) this gives |a - b| <= S * 2 * L * u * max|ref| = 6.1e-5 max|ref| per tensor, stated before any run."""
    from pn2 import F32
    from pn2.engine import Engine
    from pn2.graph import _seed_grad
    torch.manual_seed(11)
    conv = nn.Conv2d(64, 128, 1, stride=2, bias=False).to(dev)
    bn = nn.BatchNorm2d(128).to(dev)
    bn.weight.data.uniform_(0.6, 1.4); bn.bias.data.normal_(0, 0.1)
    x = torch.randn(2, 64, 8, 8, device=dev)
    gy = torch.randn(2, 128, 4, 4, device=dev)
    res = {}
    for name in ("generic", "split"):
        eng = Engine(F32, True, need_grad=True)
        a = eng.from_nchw(x, requires_grad=True)
        y = eng.conv_bn_act(a, conv, bn) if name == "generic" else eng.strided_pointwise(a, conv, bn)
        out = eng.to_nchw(y).clone()
        _seed_grad(y, gy)
        eng.backward()
        torch.cuda.synchronize()
        res[name] = dict(out=out, dx=a.grad[..., :64].permute(0, 3, 1, 2).clone(), dw=eng.pgrads.get(conv.weight).clone(), dgamma=eng.pgrads.get(bn.weight).clone(),
                         dbeta=eng.pgrads.get(bn.bias).clone())
    S_, L, u = 4, 128, 2.0 ** -24
    for k, ref in res["generic"].items():
        got = res["split"][k]
        assert got.shape == ref.shape, k
        err, bound = float((got.double() - ref.double()).abs().max()), S_ * 2 * L * u * float(ref.abs().max())
        print(f"strided_pointwise {k}: max |split - generic| {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (k, err, bound)
    assert tuple(res["split"]["out"].shape) == (2, 128, 4, 4)
    # the pixels the conv never reads: exact zeros on both paths
    off = torch.ones(8, 8, dtype=torch.bool); off[::2, ::2] = False
    assert float(res["split"]["dx"][:, :, off].abs().max()) == 0.0 and float(res["generic"]["dx"][:, :, off].abs().max()) == 0.0
    assert float(res["split"]["dx"][:, :, ::2, ::2].abs().max()) > 0


@pytest.mark.parametrize("dtn", ["bf16", "fp32"])
def test_engine_subsample_both_orders_of_arrival(dtn):
    """Engine.subsample next to a second consumer of the same activation, recorded before and after it: x's gradient is the sum either way."""
    from pn2 import F32, BF16
    from pn2.engine import Engine
    from pn2.graph import _seed_grad
    dt, tdt = (F32, torch.float32) if dtn == "fp32" else (BF16, torch.bfloat16)
    torch.manual_seed(3)
    x = torch.randn(2, 24, 7, 5, device=dev).to(tdt).float()
    g_sub, g_id = torch.randn(2, 24, 4, 3, device=dev).to(tdt).float(), torch.randn(2, 24, 7, 5, device=dev).to(tdt).float()
    want = g_id.clone(); want[:, :, ::2, ::2] += g_sub
    want = want.to(tdt).float()                                   # one rounding of the sum to the storage type
    for first in ("subsample", "other"):
        eng = Engine(dt, True, need_grad=True)
        a = eng.from_nchw(x, requires_grad=True)
        if first == "subsample":
            y, o = eng.subsample(a, 2), eng.upsample2x(a)
        else:
            o, y = eng.upsample2x(a), eng.subsample(a, 2)
        assert torch.equal(eng.to_nchw(y), x[:, :, ::2, ::2])
        _seed_grad(y, g_sub)
        # the other consumer: nearest 2x up-sampling, seeded so that its adjoint (the sum over each 2 x 2 quad) is g_id exactly (three zeros per quad)
        g_up = torch.zeros(2, 24, 14, 10, device=dev); g_up[:, :, ::2, ::2] = g_id
        _seed_grad(o, g_up)
        eng.backward()
        torch.cuda.synchronize()
        assert torch.equal(a.grad[..., :24].permute(0, 3, 1, 2).float(), want), first
