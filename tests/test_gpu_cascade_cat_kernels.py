"""GPU tests of the two kernels the concatenating CASCADE decoder adds to csrc/pn2_cascade.hip, through the C ABI against tests/cascadecatref.py in float64:
pn2_ag_apply_cat_fwd and pn2_ag_bwd_gate_cat, fed inputs that are exact in the storage type (the float64 reference reads the same values), fp32 and bf16, train- and
eval-mode BatchNorm rows, N = 2 with H x W in {1x1, 3x5, 16x16} and (C, F_int) in {(8,4), (24,12), (40,24), (64,32), (96,48)} (one vector per row up to more vectors than
a power of two), 2 x 24 x 24 with (24, 12), where the rows span several blocks (the two-phase sums), and 2 x 3 x 5 with (320, 128), the widest reference
gate: 80 fp32 vectors per row, more than the 64 lanes a row gets, so a lane walks two vectors.  F_int only names the reference stage: the psi
branch (pn2_ag_psi_fwd, pn2_ag_bwd_sum) is unchanged and stays with tests/test_gpu_cascade_kernels.py; psi_raw is an input here.
Row strides: out / dout 2 C and 2 C + 8 (the columns beyond 2 C hold a sentinel and must be untouched), g / x / dx / dg C and C + 8.

Checked: the right half of out equals g bit for bit, the left half within cascaderef's rule (one fp32 rounding per product, 2^-8 |ref| per bf16 store); dg without
accumulation equals the right half of dout bit for bit; dx, dg and dz with and without accumulation; p1 / p2 against the READ-BACK dz with the n * 2^-24 * sum|terms|
bound; two runs bit-identical; C = 12 is refused with a status and writes nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import cascaderef as R
import cascadecatref as RC

pytestmark = pytest.mark.gpu
dev = "cuda"
SENT = 7.0
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
DT = {"fp32": 0, "bf16": 1}
SHAPES = [(2, h, w, c, f) for (h, w) in ((1, 1), (3, 5), (16, 16)) for (c, f) in ((8, 4), (24, 12), (40, 24), (64, 32), (96, 48))] + [(2, 24, 24, 24, 12)] + [(2, 3, 5, 320, 128)]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()
    yield


def _lib():
    from pn2 import capi
    return capi.load()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _wide(M, C_, ld, tdt, gen, outside=float("nan")):
    """[M][ld] device buffer: C_ random columns (exact in tdt), columns beyond them `outside`; -> (buffer, float64 numpy of the random part)"""
    t = torch.full((M, ld), outside, dtype=torch.float32)
    t[:, :C_] = torch.randn(M, C_, generator=gen)
    t = t.to(tdt)
    return t.to(dev), t[:, :C_].double().numpy()


def _f32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32).reshape(-1)).to(dev)


def _close(got, ref, bound, what):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    share = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    print(f"AGC {what}: max err {float(err.max()):.3e}, share of the bound {share:.3f}")
    assert np.all(err <= bound), (what, float(err.max()), share)


@pytest.mark.parametrize("wide", [0, 8])
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_concat_gate_kernels(shape, dt, train, wide):
    lib, N, H, W, Cc, _F = _lib(), *shape
    M, tdt, bf = N * H * W, TDT[dt], dt == "bf16"
    gen = torch.Generator().manual_seed(2000 * Cc + M + (7 if train else 0))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ldc, ldo = Cc + wide, 2 * Cc + wide
    g_d, g = _wide(M, Cc, ldc, tdt, gen)
    x_d, x = _wide(M, Cc, ldc, tdt, gen)
    do_d, dout = _wide(M, 2 * Cc, ldo, tdt, gen)
    v_d = (torch.randn(M, generator=gen) * 1.5).to(dev)
    v = v_d.double().cpu().numpy()
    gam, bet, eps = 1.3, -0.2, 1e-5
    a, b, mean, invstd = R.bn1(v, gam, bet, eps, None if train else (0.1, 0.8))
    a, b = float(np.float32(a)), float(np.float32(b))
    if train:
        mean, invstd = float(np.float32(mean)), float(np.float32(invstd))
    a_d, b_d = _f32([a]), _f32([b])
    mu_d, is_d = (_f32([mean]), _f32([invstd])) if train else (None, None)
    # ---- forward (twice: bit-identical)
    outs = []
    for _ in range(2):
        o_d = torch.full((M, ldo), SENT, dtype=tdt, device=dev)
        assert lib.pn2_ag_apply_cat_fwd(DT[dt], P(g_d), ldc, P(x_d), ldc, P(v_d), P(a_d), P(b_d), P(o_d), ldo, M, Cc, Cc, st) == 0
        torch.cuda.synchronize()
        outs.append(o_d)
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0][:, Cc:2 * Cc], g_d[:, :Cc]), "the right half of a row is g, bit for bit"
    assert bool((outs[0][:, 2 * Cc:] == SENT).all())
    o = outs[0].double().cpu().numpy()
    ref = RC.apply_cat(g, x, v, a, b)
    _close(o[:, :Cc], ref[:, :Cc], RC.bound_out_left(x, v, a, b, ref[:, :Cc], bf), "out, left half")
    # ---- backward: plain and accumulating
    nb1 = lib.pn2_ag_blocks(DT[dt], M, Cc, 1)
    assert nb1 >= 1 and (M < 1000 or nb1 > 1)          # (2 x 24 x 24: several blocks in both storage types)
    rdx, rdg, rdz, _, _ = RC.bwd_gate_cat(dout, x, v, a, b, mean if train else None, invstd)
    for acc in (0, 1):
        got = []
        old_d, old = _wide(M, Cc, ldc, tdt, gen, outside=SENT)
        for _ in range(2):
            dx_d, dg_d = old_d.clone(), old_d.clone()
            dz_d, p1, p2 = torch.full((M,), float("nan"), device=dev), torch.full((nb1,), float("nan"), device=dev), torch.full((nb1,), float("nan"), device=dev)
            assert lib.pn2_ag_bwd_gate_cat(DT[dt], P(do_d), ldo, P(x_d), ldc, P(v_d), P(a_d), P(b_d), P(mu_d), P(is_d), P(dx_d), ldc, acc, P(dg_d), ldc, acc,
                                           P(dz_d), P(p1), P(p2), M, Cc, Cc, st) == 0
            torch.cuda.synchronize()
            got.append((dx_d, dg_d, dz_d, p1, p2))
        assert all(torch.equal(u, v_) for u, v_ in zip(got[0], got[1]))
        if not acc:
            assert torch.equal(got[0][1][:, :Cc], do_d[:, Cc:2 * Cc]), "dg without accumulation is the right half of dout, bit for bit"
        dx_g, dg_g, dz_g = (t.double().cpu().numpy() for t in got[0][:3])
        o64 = old * acc
        _close(dx_g[:, :Cc], rdx + o64, R.bound_dx(dout[:, :Cc], v, a, b, rdx + o64, o64, bf), f"dx acc={acc}")
        _close(dg_g[:, :Cc], rdg + o64, RC.bound_dg(rdg, o64, acc, bf), f"dg acc={acc}")
        assert np.all(dx_g[:, Cc:] == SENT) and np.all(dg_g[:, Cc:] == SENT)
        _close(dz_g, rdz, R.bound_dz(dout[:, :Cc], x, v, a, b, Cc), f"dz acc={acc}")
        xh = (v - mean) * invstd if train else np.zeros(M)
        _close(float(got[0][3].double().sum()), dz_g.sum(), (M + nb1) * R.E * np.abs(dz_g).sum() + 1e-30, "p1 (dbeta)")
        _close(float(got[0][4].double().sum()), (dz_g * xh).sum(), (M + nb1 + 3) * R.E * (np.abs(dz_g) * (np.abs(v) + abs(mean or 0.0)) * (invstd or 0.0)).sum() + 1e-30, "p2 (dgamma)")
    # ---- null dx / dg: the other one and dz are written all the same
    dg_d = torch.full((M, ldc), SENT, dtype=tdt, device=dev)
    dz2, p1, p2 = torch.zeros(M, device=dev), torch.zeros(nb1, device=dev), torch.zeros(nb1, device=dev)
    z = C.c_void_p(0)
    assert lib.pn2_ag_bwd_gate_cat(DT[dt], P(do_d), ldo, P(x_d), ldc, P(v_d), P(a_d), P(b_d), P(mu_d), P(is_d), z, 0, 0, P(dg_d), ldc, 0, P(dz2), P(p1), P(p2), M, Cc, Cc, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(dg_d[:, :Cc], do_d[:, Cc:2 * Cc]) and torch.equal(dz2, got[0][2])


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_concat_gate_entry_points_refuse(dt):
    """-1 for a null argument, -2 for a width that is no multiple of 8 (padded or not), rows too narrow or not 16-byte aligned; nothing is written."""
    lib = _lib()
    t = torch.zeros(64, 64, dtype=TDT[dt], device=dev)
    o = torch.full((64, 64), SENT, dtype=TDT[dt], device=dev)
    v = torch.full((64,), SENT, device=dev)
    z, d = C.c_void_p(0), DT[dt]
    assert lib.pn2_ag_apply_cat_fwd(d, P(t), 64, P(t), 64, P(v), z, P(v), P(o), 64, 64, 16, 16, z) == -1
    assert lib.pn2_ag_apply_cat_fwd(d, P(t), 64, P(t), 64, P(v), P(v), P(v), P(o), 64, 64, 12, 16, z) == -2          # C = 12 in 16 slots
    assert lib.pn2_ag_apply_cat_fwd(d, P(t), 64, P(t), 64, P(v), P(v), P(v), P(o), 64, 64, 12, 12, z) == -2          # C = 12, unpadded
    assert lib.pn2_ag_apply_cat_fwd(d, P(t), 64, P(t), 64, P(v), P(v), P(v), P(o), 24, 64, 16, 16, z) == -2          # a row of out below 2 C
    assert lib.pn2_ag_apply_cat_fwd(d, P(t), 64, P(t), 18, P(v), P(v), P(v), P(o), 64, 64, 16, 16, z) == -2          # rows not 16-byte aligned
    for args in ((12, 16), (12, 12)):
        assert lib.pn2_ag_bwd_gate_cat(d, P(t), 64, P(t), 64, P(v), P(v), P(v), z, z, P(o), 64, 0, P(o), 64, 0, P(v), P(v), P(v), 64, *args, z) == -2
    assert lib.pn2_ag_bwd_gate_cat(d, P(t), 64, P(t), 64, P(v), P(v), P(v), z, z, P(o), 64, 0, P(o), 64, 0, z, P(v), P(v), 64, 16, 16, z) == -1
    assert lib.pn2_ag_bwd_gate_cat(d, P(t), 24, P(t), 64, P(v), P(v), P(v), z, z, P(o), 64, 0, P(o), 64, 0, P(v), P(v), P(v), 64, 16, 16, z) == -2      # a row of dout below 2 C
    assert lib.pn2_ag_bwd_gate_cat(d, P(t), 64, P(t), 64, P(v), P(v), P(v), P(v), z, P(o), 64, 0, P(o), 64, 0, P(v), P(v), P(v), 64, 16, 16, z) == -1    # mean without invstd
    torch.cuda.synchronize()
    assert bool((v == SENT).all()) and bool((o == SENT).all()) and bool((t == 0).all())
