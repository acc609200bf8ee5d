"""The fp32x3 conv kernels (PN2_F32X3) one by one at the C ABI, on plain fp32 operands, against the float64 contraction of the same operands: the geometry
sweep of tests/test_gpu_convkernels_fp32.py run in the new mode.  Its test bodies are reused as they are; for the duration of each test here, the
mode table, the gate of a conv output (check), the gate of a weight gradient (_wgrad_check), the row-tile rule (_tile_m: fp32x3 takes the BM / BN bits
of a tuning code like fp32fast) and the worst-case gate the epilogue tests read from fp32ref are pointed at fp32x3's (tests/fp32x3ref.py):
  worst case |got - r| <= gate_fp32x3(S, K) + 1/2 ulp (weight gradients: wgrad_tol_x3), and rms(got - r) <= 2 rms(ref32 - r), ref32 = torch's CPU float32
  conv of the same operands; the rms gate is checked >= 10 x tighter than the error of bf16 operands on every output.
Plus: NaN inside the read channels reaches the same outputs as in fp32, and an entry point outside the conv contraction set returns -3 for code 3."""
import ctypes as C
import os, sys, types

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "pranet-v2_amd"))
import fp32ref as R  # noqa: E402
import fp32x3ref as X  # noqa: E402
import test_gpu_convkernels_fp32 as T  # noqa: E402

dev = "cuda"
MODE = "F32X3"


def _check_x3(mode, got, r, S, K, ref32=None, extra=None, canary=None, what=""):
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output (a tile was not written, or NaN reached it)"
    err = (got - r).abs()
    tol = X.gate_fp32x3(S, K) + 0.5 * R.spacing32(got)
    if extra is not None:
        tol = tol + extra
    bad = err > tol
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the fp32x3 gate, worst excess {float((err - tol).max()):.3g}"
    ratio = None
    if ref32 is not None:
        own = R.rms(ref32 - r)
        ratio = R.rms(got - r) / own
        print(f"{what}: rms(got - r) / rms(ref32 - r) = {ratio:.3f}")
        assert ratio <= 2.0, (what, ratio)
        if canary is not None:
            T._canary(2 * own, *canary)
    elif canary is not None:
        T._canary(R.rms(tol), *canary)
    return ratio


def _wgrad_check_x3(mode, gw, slab, ns, ref, S, ref32, M, what, canary=None):
    Cout, Cin, KH, KW = gw.shape
    got = gw.double().cpu().permute(0, 2, 3, 1).reshape(Cout, KH * KW * Cin)
    sl = slab.double().cpu()[:, :Cout, :KH * KW * Cin]
    assert bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    tol = X.wgrad_tol_x3(got, sl, ns, S, M)
    bad = err > tol
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} outside the fp32x3 gate, worst excess {float((err - tol).max()):.3g}"
    if ref32 is not None:
        own = R.rms(ref32 - ref)
        ratio = R.rms(got - ref) / own
        print(f"{what}: rms(got - r) / rms(ref32 - r) = {ratio:.3f}")
        assert ratio <= 2.0, (what, ratio)
        if canary is not None:
            T._canary(2 * own, *canary)


@pytest.fixture(autouse=True)
def _x3(monkeypatch):
    """point the shared test bodies at fp32x3 for this test only (undone afterwards)"""
    from pn2 import capi
    mode0, tile0 = T._mode, T._tile_m
    monkeypatch.setattr(T, "_mode", lambda name: capi.F32X3 if name == MODE else mode0(name))
    monkeypatch.setattr(T, "_tile_m", lambda mode, code, M, n_out: tile0("F32F" if mode == MODE else mode, code, M, n_out))
    monkeypatch.setattr(T, "check", _check_x3)
    monkeypatch.setattr(T, "_wgrad_check", _wgrad_check_x3)
    proxy = types.SimpleNamespace(**{k: getattr(R, k) for k in dir(R) if not k.startswith("__")})
    proxy.gate_fp32fast = lambda S, K, chain=16: X.gate_fp32x3(S, K)
    monkeypatch.setattr(T, "R", proxy)
    yield


@pytest.mark.parametrize("slices", [0, 1], ids=["dense", "slices"])
@pytest.mark.parametrize("geom", T.GEOMS, ids=T._ids(T.GEOMS))
@pytest.mark.parametrize("transposed", [0, 1], ids=["fwd", "dgrad"])
def test_gather_gemm_every_tile_code_against_float64(transposed, geom, slices):
    T.test_gather_gemm_every_tile_code_against_float64(MODE, transposed, geom, slices)


@pytest.mark.parametrize("geom", T.WGEOMS, ids=T._ids(T.WGEOMS))
def test_wgrad_splits_and_tunes_against_float64(geom):
    T.test_wgrad_splits_and_tunes_against_float64(MODE, geom)


@pytest.mark.parametrize("form", T.EP_FORMS)
def test_dgrad_batchnorm_backward_epilogue_against_float64(form):
    T.test_dgrad_batchnorm_backward_epilogue_against_float64(MODE, form)


def test_gated_and_affine_epilogues_against_float64():
    T.test_gated_and_affine_epilogues_against_float64(MODE)


def test_table_launches_match_single_launches_bitwise():
    T.test_table_launches_match_single_launches_bitwise(MODE)


@pytest.mark.parametrize("geom", [(2, 11, 13, 72, 40, 1, 1, 1, 0, 0, 1), (2, 11, 13, 104, 104, 3, 3, 1, 1, 1, 1), (2, 16, 18, 56, 56, 3, 3, 2, 1, 1, 1)],
                         ids=["1x1", "3x3", "3x3s2"])
@pytest.mark.parametrize("transposed", [0, 1], ids=["fwd", "dgrad"])
def test_nan_channels_reach_the_same_outputs_as_fp32(transposed, geom):
    """NaN in read channels of some input pixels: fp32x3 (h = NaN, r = NaN - NaN) gives NaN exactly where the fp32 parity path does, finite values
    elsewhere within the gate"""
    from pn2 import capi
    lib = T._lib()
    d, src, wp, n_out, M, ld_out, a, b, ref32, K = T._setup(geom, transposed, MODE, 0, 11)
    g = torch.Generator().manual_seed(3)
    rows = torch.randint(0, src.shape[0], (3,), generator=g)
    chans = torch.randint(0, d.Cin_p, (3,), generator=g)
    src[rows.to(dev), chans.to(dev)] = float("nan")
    outs = {}
    for dt in (capi.F32, capi.F32X3):
        out = torch.zeros(M, ld_out, device=dev)
        assert lib.pn2_conv_gemm(dt, T.P(src), T.P(wp), T.P(out), T.P(None), T.P(None), C.byref(d), T._stream()) == 0
        torch.cuda.synchronize()
        outs[dt] = out[:, :n_out].double().cpu()
    n32, nx3 = torch.isnan(outs[capi.F32]), torch.isnan(outs[capi.F32X3])
    assert bool(n32.any()) and torch.equal(n32, nx3)
    fin = ~n32
    S = a.abs().nan_to_num(0) @ b.abs().t()
    assert bool(((outs[capi.F32X3] - outs[capi.F32]).abs()[fin] <= (X.gate_fp32x3(S, K) + R.spacing32(outs[capi.F32]))[fin]).all())


def test_entry_points_outside_the_conv_contractions_refuse_code_3():
    from pn2 import capi
    lib = T._lib()
    p = capi.PackDesc() if hasattr(capi, "PackDesc") else None
    w = torch.zeros(64, device=dev)
    if p is not None:
        p.Cout, p.Cin, p.KH, p.KW, p.Cout_p, p.gw_out, p.gwp_out, p.Cin_p, p.gw_in, p.gwp_in, p.Rp, p.Kp = 1, 1, 1, 1, 8, 1, 1, 8, 1, 1, 128, 128
        assert lib.pn2_pack_weight(capi.F32X3, T.P(w), T.P(w), C.byref(p), T._stream()) == -3
    assert lib.pn2_depth_to_space(capi.F32X3, T.P(w), 8, T.P(w), 8, 1, 2, 2, 1, 1, 2, 8, 0, T._stream()) == -3
    # and the contraction entry points accept it: same tiles / statistics blocks as fp32fast
    for m, co in ((100, 40), (5000, 64), (70000, 256)):
        assert lib.pn2_conv_tile_m(m, co, capi.F32X3) == lib.pn2_conv_tile_m(m, co, capi.F32F)
        assert lib.pn2_conv_stat_blocks(m, co, capi.F32X3) == lib.pn2_conv_stat_blocks(m, co, capi.F32F)
