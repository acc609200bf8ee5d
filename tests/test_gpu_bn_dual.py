"""GPU tests of the two-BatchNorm passes of a Bottle2neck stage block (pn2_bn.hip): pn2_affine_act_dual, the output pass out = relu(bn3(raw3) + T(bn_d(raw_d))) that never
writes the downsample BatchNorm's output, and pn2_bn_bwd_apply_dual, the backward apply pass that reads the masked gradient once for both BatchNorms.

Both replace two launches of an existing kernel and promise their bits, so the first reference is those two launches.  The dual normalise pass is also held to the float64
formula with the storage rounding where the two launches apply it (the intermediate is stored, so it is rounded to the storage dtype): tests/test_gpu_spatial_kernels.py has
no normalise case of its own, its rule for an element-wise result that adds two terms is used - 2^-23 * (|a| + |b|) per element (one rounding of the fused multiply-add, one
of the sum) and for bf16 the half ulp 2^-8 * |ref| of the final store.

Shapes: M is no multiple of the rows per block (256 / CVP) nor of the row unroll, the channel counts are no powers of two (lanes beyond the last channel vector idle), every
tensor is a slice of a wider buffer and x2 has a leading dimension of its own.  Pads and a guard row hold a sentinel that has to survive.

The end-to-end cases run Bottle2neck blocks through run_module with the switches PN2_DUAL_AFFINE / PN2_DUAL_BNB_APPLY on and off: outputs, input and parameter gradients
bit-identical.  One stage block alone receives its output gradient from autograd, so no dgrad epilogue leaves the sums the dual apply pass needs and it must not run; in the
two-block case (stage block + normal block) conv1's dgrad of the second block completes that gradient.  Its epilogue leaves both BatchNorms' sums for tiles of <= 4096
elements only, and the tile is otherwise the tuner's timed choice, so the test pins that one launch (the only dgrad with an epilogue onto a 64-channel input) to the 64 x 64
tile of the LDS-DMA kernel: the dual apply pass then has to run exactly once when its switch is on and never when it is off."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
IDT = {"fp32": torch.int32, "bf16": torch.int16}
DT = {"fp32": 0, "bf16": 1}
SENT = 7.0
SHAPES = [(2 * 5 * 7, 40), (1 * 9 * 9, 104), (3 * 4 * 4, 256)]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()
    yield
    pn2.set_compute_dtype("bf16")


def _lib():
    from pn2 import capi
    return capi.load()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _buf(M, Cc, ld, dt, body=None):
    """[M + 1][ld] rows, body in [:M, :C], sentinel in the pads and the guard row (NaN body when none is given: an output)."""
    t = torch.full((M + 1, ld), SENT, dtype=TDT[dt])
    t[:M, :Cc] = float("nan") if body is None else body.to(TDT[dt])
    return t.to(dev)


def _bits(t, dt):
    return t.contiguous().view(IDT[dt]).cpu()


def _pads_ok(t, M, Cc, dt):
    ref = torch.full_like(t, SENT)
    return torch.equal(_bits(t[:M, Cc:], dt), _bits(ref[:M, Cc:], dt)) and torch.equal(_bits(t[M], dt), _bits(ref[M], dt))


def _rows(g, n, lo=0.5, hi=1.5):
    return (torch.rand(n, generator=g) * (hi - lo) + lo).float()


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("M,Cc", SHAPES, ids=[f"{m}x{c}" for m, c in SHAPES])
def test_dual_affine_equals_two_launches_bitwise(M, Cc, dt, relu):
    lib, g = _lib(), torch.Generator().manual_seed(100 * M + Cc + relu)
    ld_x, ld_x2, ld_y = Cc + 8, Cc + 24, Cc + 16
    xb = torch.randn(M, Cc, generator=g).to(TDT[dt])
    x2b = (torch.randn(M, Cc, generator=g) * 2 - 0.3).to(TDT[dt])
    sc, sh, sc2, sh2 = _rows(g, Cc), _rows(g, Cc, -0.5, 0.5), _rows(g, Cc, -1.5, 1.5), _rows(g, Cc, -0.5, 0.5)
    x, x2 = _buf(M, Cc, ld_x, dt, xb), _buf(M, Cc, ld_x2, dt, x2b)
    par = [t.to(dev) for t in (sc, sh, sc2, sh2)]
    tmp, y_two, y_one = _buf(M, Cc, Cc, dt), _buf(M, Cc, ld_y, dt), _buf(M, Cc, ld_y, dt)
    assert lib.pn2_affine_act(DT[dt], _p(x2), ld_x2, DT[dt], _p(tmp), Cc, M, Cc, _p(par[2]), _p(par[3]), None, 0, 0, _st()) == 0
    assert lib.pn2_affine_act(DT[dt], _p(x), ld_x, DT[dt], _p(y_two), ld_y, M, Cc, _p(par[0]), _p(par[1]), _p(tmp), Cc, relu, _st()) == 0
    assert lib.pn2_affine_act_dual(DT[dt], _p(x), ld_x, _p(par[0]), _p(par[1]), _p(x2), ld_x2, _p(par[2]), _p(par[3]), _p(y_one), ld_y, M, Cc, relu, _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(y_one, dt), _bits(y_two, dt))
    assert _pads_ok(y_one, M, Cc, dt)
    # float64 formula; the intermediate is rounded where the two launches store it (fp32 result of the fused multiply-add, then the storage dtype)
    a = xb.double() * sc.double() + sh.double()
    r = (x2b.double() * sc2.double() + sh2.double()).float().to(TDT[dt]).double()
    ref = a + r
    if relu:
        ref = ref.clamp_min(0)
    ours = y_one[:M, :Cc].cpu().double()
    bound = 2.0 ** -23 * (a.abs() + r.abs())
    if dt == "bf16":
        bound = bound + 2.0 ** -8 * (ref.abs() + bound)          # the store rounds the computed value, which is within the fp32 bound of ref
    ratio = float(((ours - ref).abs() / bound.clamp_min(1e-300)).max())
    print(f"\nBNDUAL affine {M}x{Cc} {dt} relu{relu}: max err {float((ours - ref).abs().max()):.2e} of-bound {ratio:.3f}")
    assert torch.isfinite(ours).all() and ratio <= 1.0


def test_dual_affine_refuses_unaligned_rows():
    lib, one = _lib(), C.c_void_p(256)
    assert lib.pn2_affine_act_dual(1, one, 40, one, one, one, 44, one, one, one, 40, 8, 40, 1, None) == -2
    assert lib.pn2_affine_act_dual(1, one, 40, one, one, None, 40, one, one, one, 40, 8, 40, 1, None) == -1
    assert lib.pn2_bn_bwd_apply_dual(1, one, 40, 8, 40, one, 40, one, one, one, one, 40, one, 42, one, one, one, one, 40, None) == -2
    assert lib.pn2_bn_bwd_apply_dual(1, one, 40, 8, 40, one, 40, one, one, None, one, 40, one, 40, one, one, one, one, 40, None) == -1


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("M,Cc", SHAPES, ids=[f"{m}x{c}" for m, c in SHAPES])
def test_dual_apply_equals_two_launches_bitwise(M, Cc, dt):
    lib, g = _lib(), torch.Generator().manual_seed(7 * M + Cc)
    npad = 6          # the last channels are pad slots: every parameter row is zero there, as the finalize kernels leave them
    ld_dz, ld_xa, ld_xb, ld_da, ld_db = Cc + 8, Cc + 16, Cc + 24, Cc, Cc + 8
    dzb = torch.randn(M, Cc, generator=g)
    dzb[torch.rand(M, Cc, generator=g) < 0.4] = 0.0          # where the producer's ReLU mask was off
    dz = _buf(M, Cc, ld_dz, dt, dzb)
    xs, pars = [], []
    for k in range(2):
        xs.append(_buf(M, Cc, (ld_xa, ld_xb)[k], dt, torch.randn(M, Cc, generator=g) + 0.3 * k))
        mean, invstd = _rows(g, Cc, -0.5, 0.5), _rows(g, Cc, 0.5, 2.0)
        coef = torch.stack([_rows(g, Cc, 0.2, 2.0), _rows(g, Cc, -0.1, 0.1), _rows(g, Cc, -0.1, 0.1)])
        mean[-npad:], invstd[-npad:], coef[:, -npad:] = 0.0, 0.0, 0.0
        pars.append((mean.to(dev), invstd.to(dev), coef.contiguous().to(dev)))
    two = [_buf(M, Cc, ld_da, dt), _buf(M, Cc, ld_db, dt)]
    one = [_buf(M, Cc, ld_da, dt), _buf(M, Cc, ld_db, dt)]
    for k in range(2):
        assert lib.pn2_bn_bwd_apply(DT[dt], DT[dt], _p(dz), ld_dz, Cc, None, 0, DT[dt], _p(xs[k]), (ld_xa, ld_xb)[k], M, Cc, _p(pars[k][0]), _p(pars[k][1]), _p(pars[k][2]),
                                    _p(two[k]), (ld_da, ld_db)[k], None, 0, 0, None, None, 0, _st()) == 0
    assert lib.pn2_bn_bwd_apply_dual(DT[dt], _p(dz), ld_dz, M, Cc, _p(xs[0]), ld_xa, _p(pars[0][0]), _p(pars[0][1]), _p(pars[0][2]), _p(one[0]), ld_da,
                                     _p(xs[1]), ld_xb, _p(pars[1][0]), _p(pars[1][1]), _p(pars[1][2]), _p(one[1]), ld_db, _st()) == 0
    torch.cuda.synchronize()
    for k in range(2):
        assert torch.equal(_bits(one[k], dt), _bits(two[k], dt)), k
        assert _pads_ok(one[k], M, Cc, dt) and torch.isfinite(one[k][:M, :Cc]).all()
        assert float(one[k][:M, Cc - npad:Cc].abs().max()) == 0.0          # pad channels: zero gradient


def _blocks(n_blocks):
    from lib.Res2Net_v1b import Bottle2neck
    torch.manual_seed(3)
    down = torch.nn.Sequential(torch.nn.AvgPool2d(kernel_size=2, stride=2, ceil_mode=True, count_include_pad=False),
                               torch.nn.Conv2d(64, 64, kernel_size=1, stride=1, bias=False), torch.nn.BatchNorm2d(64))
    blocks = [Bottle2neck(64, 16, stride=2, downsample=down, stype='stage')] + [Bottle2neck(64, 16) for _ in range(n_blocks - 1)]
    m = torch.nn.Sequential(*blocks)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.copy_(torch.rand_like(p) + 0.5)          # BatchNorm weights and biases away from their 1 / 0 defaults
    return m.to(dev).train()


PIN_64x64 = 3 | (1 << 2) | (2 << 4)          # tuning code: LDS-DMA kernel with a 2-stage ring, 64-row x 64-column tile


def _run_blocks(n_blocks, monkeypatch, **switches):
    import pn2
    from pn2 import core
    from pn2.ops_conv import ConvOps
    from pn2.capi import call
    from pn2.graph import run_module
    pn2.set_compute_dtype("bf16")
    for k, v in switches.items():
        assert hasattr(core, k), k
        monkeypatch.setattr(core, k, v)
    real_tune = ConvOps._tune_gemm
    monkeypatch.setattr(ConvOps, "_tune_gemm", lambda self, cd, in_ptr, wp, M, Cout, ep=None: PIN_64x64 if (ep is not None and Cout == 64) else real_tune(self, cd, in_ptr, wp, M, Cout, ep))
    m = _blocks(n_blocks)
    x = torch.randn(2, 64, 12, 12, generator=torch.Generator().manual_seed(5)).to(dev).requires_grad_(True)
    counts = {}
    for name in ("pn2_affine_act_dual", "pn2_bn_bwd_apply_dual"):
        real = getattr(call, name)
        monkeypatch.setattr(call, name, lambda *a, _n=name, _r=real: (counts.__setitem__(_n, counts.get(_n, 0) + 1), _r(*a))[1])

    def build(e, a):
        for b in m:
            a = b._build(e, a)
        return [a]
    y = run_module(build, [x], list(m.parameters()), True)[0]
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(6)).to(dev)
    (y * gy).sum().backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    return [y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in m.parameters()], counts


@pytest.mark.parametrize("n_blocks", [1, 2], ids=["stage", "stage+normal"])
def test_stage_block_switches_are_bit_identical(n_blocks, monkeypatch):
    off, c_off = _run_blocks(n_blocks, monkeypatch, DUAL_AFFINE=False, DUAL_BNB_APPLY=False)
    on, c_on = _run_blocks(n_blocks, monkeypatch)
    print(f"\nBNDUAL blocks {n_blocks}: dual launches off {c_off} on {c_on}")
    assert not c_off and c_on.get("pn2_affine_act_dual") == 1
    assert c_on.get("pn2_bn_bwd_apply_dual", 0) == n_blocks - 1          # one stage block alone: no dgrad epilogue, no dual apply; behind a second block: exactly once
    assert len(on) == len(off)
    for k, (a, b) in enumerate(zip(on, off)):
        assert torch.isfinite(a).all() and torch.equal(a, b), k
    # each switch on its own
    for sw in ("DUAL_AFFINE", "DUAL_BNB_APPLY"):
        one, c_one = _run_blocks(n_blocks, monkeypatch, **{sw: False})
        assert c_one.get("pn2_affine_act_dual", 0) == (0 if sw == "DUAL_AFFINE" else 1), (sw, c_one)
        assert c_one.get("pn2_bn_bwd_apply_dual", 0) == (0 if sw == "DUAL_BNB_APPLY" else n_blocks - 1), (sw, c_one)
        for k, (a, b) in enumerate(zip(one, off)):
            assert torch.equal(a, b), (sw, k)
