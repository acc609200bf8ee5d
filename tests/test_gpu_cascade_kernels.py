"""GPU tests of csrc/pn2_cascade.hip through the C ABI against tests/cascaderef.py in float64: pn2_ag_psi_fwd, pn2_ag_apply_fwd, pn2_ag_bwd_gate, pn2_ag_bwd_sum, each fed
inputs that are exact in its storage type (the float64 reference reads the same values), fp32 and bf16, train- and eval-mode BatchNorm, rows of g / x / dout as wide as
the tensor and wider (a slice of a concat buffer), N = 2 with H x W in {1x1, 3x5, 16x16} and (C, F_int) in {(8,4), (12,6), (24,12), (64,32), (96,48)} (pad lanes at both widths, a
width below one vector), and 2 x 24 x 24 with (24, 12), where every kernel's rows span several blocks (the two-phase sums).

Checked: psi_raw and the per-block (mean, M2) that pn2_bn_finalize takes, against the READ-BACK psi_raw; out; dx and dg with and without accumulation; dz and the sums
p1 / p2 (the BatchNorm-psi parameter gradients) against the read-back dz; the ReLU-sum gradient dsum; the partial rows of dw_psi and db_psi; pad lanes exactly zero, the
columns beyond Cp of a wide row untouched; two runs bit-identical.  Bounds: cascaderef's docstring (n * 2^-24 * sum|terms| per fp32 accumulation, 2^-8 |ref| per bf16
store; where the ReLU's argument is below its own fp32 error the mask-dependent outputs are not compared)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cascaderef as R

pytestmark = pytest.mark.gpu
dev = "cuda"
SENT = 7.0
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
DT = {"fp32": 0, "bf16": 1}
SHAPES = [(2, h, w, c, f) for (h, w) in ((1, 1), (3, 5), (16, 16)) for (c, f) in ((8, 4), (12, 6), (24, 12), (64, 32), (96, 48))] + [(2, 24, 24, 24, 12)]


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


def rup8(v):
    return (v + 7) // 8 * 8


def _wide(M, C_, Cp, ld, tdt, gen, scale=1.0, pad=0.0, outside=float("nan")):
    """[M][ld] device buffer: logical columns random (exact in tdt), pad lanes `pad`, columns beyond Cp `outside`; -> (buffer, float64 numpy of the logical + pad part)"""
    t = torch.full((M, ld), outside, dtype=torch.float32)
    t[:, :Cp] = pad
    t[:, :C_] = torch.randn(M, C_, generator=gen) * scale
    t = t.to(tdt)
    return t.to(dev), t[:, :Cp].double().numpy()


def _f32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32).reshape(-1)).to(dev)


def _close(got, ref, bound, what):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    share = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    print(f"AGK {what}: max err {float(err.max()):.3e}, share of the bound {share:.3f}")
    assert np.all(err <= bound), (what, float(err.max()), share)


@pytest.mark.parametrize("wide", [0, 16])
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attention_gate_kernels(shape, dt, train, wide):
    lib, N, H, W, Cc, F = _lib(), *shape
    M, Cp, Fp, tdt, bf = N * H * W, rup8(Cc), rup8(F), TDT[dt], dt == "bf16"
    gen = torch.Generator().manual_seed(1000 * Cc + M + (7 if train else 0))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ldc, ldf = Cp + wide, Fp + wide
    # ---- operands
    rg_d, rg = _wide(M, F, Fp, ldf, tdt, gen)
    rx_d, rx = _wide(M, F, Fp, ldf, tdt, gen)
    g_d, g = _wide(M, Cc, Cp, ldc, tdt, gen)
    x_d, x = _wide(M, Cc, Cp, ldc, tdt, gen)
    do_d, dout_all = _wide(M, Cc, Cp, ldc, tdt, gen, pad=3.0)          # a gradient buffer's pad lanes hold anything finite
    dout = dout_all.copy(); dout[:, Cc:] = 0.0
    rows = np.zeros((4, Fp)); rows[:, :F] = (torch.randn(4, F, generator=gen) * 0.5 + torch.tensor([[1.0], [0.0], [1.0], [0.0]])).float().double().numpy()
    w = (torch.randn(F, generator=gen) * 0.5).float()
    rows_d, w_d = _f32(rows), w.to(dev)
    sg, hg, sx, hx = (rows_d[i * Fp:(i + 1) * Fp] for i in range(4))
    w64 = np.zeros(Fp); w64[:F] = w.double().numpy()
    s, T, arg = R.relu_sum(rg, rows[0], rows[1], rx, rows[2], rows[3])
    # ---- psi forward (twice: bit-identical)
    nb = lib.pn2_ag_blocks(DT[dt], M, Fp, 0); rpb = lib.pn2_ag_psi_rows(DT[dt], M, Fp)
    assert nb == (M + rpb - 1) // rpb
    res = []
    for _ in range(2):
        v_d, pm, pq = torch.full((M,), float("nan"), device=dev), torch.full((nb,), float("nan"), device=dev), torch.full((nb,), float("nan"), device=dev)
        rc = lib.pn2_ag_psi_fwd(DT[dt], P(rg_d), ldf, P(sg), P(hg), P(rx_d), ldf, P(sx), P(hx), P(w_d), F, Fp, M, P(v_d), P(pm if train else None), P(pq if train else None), st)
        assert rc == 0
        torch.cuda.synchronize()
        res.append((v_d.clone(), pm.clone(), pq.clone()))
    assert torch.equal(res[0][0], res[1][0]) and (not train or (torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])))
    v_got = res[0][0].double().cpu().numpy()
    _close(v_got, s @ w64, R.bound_psi_raw(T, w64), "psi_raw")
    if train:
        for b_ in range(nb):
            blk = v_got[b_ * rpb:(b_ + 1) * rpb]
            n = len(blk)
            _close(float(res[0][1][b_]), blk.mean(), (n + 1) * R.E * np.abs(blk).sum() / n, f"block mean {b_}")
            dl = np.abs(blk - blk.mean())
            _close(float(res[0][2][b_]), (dl ** 2).sum(), (n + 3) * R.E * (dl ** 2).sum() + 2 * (dl * (n + 2) * R.E * np.abs(blk).mean()).sum() + 1e-30, f"block M2 {b_}")
    # ---- the one-channel BatchNorm rows, from the kernel's psi_raw (fp32 values, exact inputs of the next kernels)
    gam, bet, eps = 1.3, -0.2, 1e-5
    a, b, mean, invstd = R.bn1(v_got, gam, bet, eps, None if train else (0.1, 0.8))
    a, b = float(np.float32(a)), float(np.float32(b))
    if train:
        mean, invstd = float(np.float32(mean)), float(np.float32(invstd))
    a_d, b_d = _f32([a]), _f32([b])
    mu_d, is_d = (_f32([mean]), _f32([invstd])) if train else (None, None)
    # ---- apply
    outs = []
    for _ in range(2):
        o_d = torch.full((M, ldc), SENT, dtype=tdt, device=dev)
        assert lib.pn2_ag_apply_fwd(DT[dt], P(g_d), ldc, P(x_d), ldc, P(res[0][0]), P(a_d), P(b_d), P(o_d), ldc, M, Cc, Cp, st) == 0
        torch.cuda.synchronize()
        outs.append(o_d)
    assert torch.equal(outs[0], outs[1])
    o = outs[0].double().cpu().numpy()
    ref = R.apply(g, x, v_got, a, b)
    _close(o[:, :Cc], ref[:, :Cc], R.bound_out(g, x, v_got, a, b, ref, bf)[:, :Cc], "out")
    assert np.all(o[:, Cc:Cp] == 0.0) and np.all(o[:, Cp:] == SENT)
    # ---- backward, gate half: plain and accumulating
    nb1 = lib.pn2_ag_blocks(DT[dt], M, Cp, 1)
    rdx, rdg, rdz, _, _ = R.bwd_gate(dout, x, v_got, a, b, mean if train else None, invstd)
    for acc in (0, 1):
        got = []
        old_d, old = _wide(M, Cc, Cp, ldc, tdt, gen, outside=SENT)
        for _ in range(2):
            dx_d, dg_d = old_d.clone(), old_d.clone()
            dz_d, p1, p2 = torch.full((M,), float("nan"), device=dev), torch.full((nb1,), float("nan"), device=dev), torch.full((nb1,), float("nan"), device=dev)
            assert lib.pn2_ag_bwd_gate(DT[dt], P(do_d), ldc, P(x_d), ldc, P(res[0][0]), P(a_d), P(b_d), P(mu_d), P(is_d), P(dx_d), ldc, acc, P(dg_d), ldc, acc,
                                       P(dz_d), P(p1), P(p2), M, Cc, Cp, st) == 0
            torch.cuda.synchronize()
            got.append((dx_d, dg_d, dz_d, p1, p2))
        assert all(torch.equal(u, v_) for u, v_ in zip(got[0], got[1]))
        dx_g, dg_g, dz_g = (t.double().cpu().numpy() for t in got[0][:3])
        o64 = old * acc
        _close(dx_g[:, :Cc], (rdx + o64)[:, :Cc], R.bound_dx(dout, v_got, a, b, rdx + o64, o64, bf)[:, :Cc], f"dx acc={acc}")
        _close(dg_g[:, :Cc], (rdg + o64)[:, :Cc], (R.E * (np.abs(rdg) + np.abs(o64)) * acc + R.bound_store(rdg + o64, bf) * acc)[:, :Cc], f"dg acc={acc}")
        assert np.all(dx_g[:, Cc:Cp] == 0.0) and np.all(dg_g[:, Cc:Cp] == 0.0) and np.all(dx_g[:, Cp:] == SENT) and np.all(dg_g[:, Cp:] == SENT)
        _close(dz_g, rdz, R.bound_dz(dout, x, v_got, a, b, Cp), f"dz acc={acc}")
        xh = (v_got - mean) * invstd if train else np.zeros(M)
        _close(float(got[0][3].double().sum()), dz_g.sum(), (M + nb1) * R.E * np.abs(dz_g).sum() + 1e-30, "p1 (dbeta)")
        _close(float(got[0][4].double().sum()), (dz_g * xh).sum(), (M + nb1 + 3) * R.E * (np.abs(dz_g) * (np.abs(v_got) + abs(mean or 0.0)) * (invstd or 0.0)).sum() + 1e-30, "p2 (dgamma)")
    # ---- backward, ReLU-sum half
    nb2 = lib.pn2_ag_blocks(DT[dt], M, Fp, 2)
    coef = (float(np.float32(gam * invstd)), float(np.float32(dz_g.mean())), float(np.float32((dz_g * xh).mean()))) if train else None
    coef_d = _f32(coef) if train else None
    rdp, rds, rdw, rdb = R.bwd_sum(dz_g, v_got, a, mean, invstd, coef, s, w64)
    e_dp = R.bound_dp(dz_g, v_got, mean, invstd, coef, a)
    got = []
    for _ in range(2):
        ds_d = torch.full((M, ldf), SENT, dtype=tdt, device=dev)
        pw, pb = torch.full((nb2, Fp), float("nan"), device=dev), torch.full((nb2,), float("nan"), device=dev)
        assert lib.pn2_ag_bwd_sum(DT[dt], P(dz_d), P(res[0][0]), P(a_d), P(mu_d), P(is_d), P(coef_d), P(rg_d), ldf, P(sg), P(hg), P(rx_d), ldf, P(sx), P(hx),
                                  P(w_d), F, Fp, M, P(ds_d), ldf, P(pw), P(pb), st) == 0
        torch.cuda.synchronize()
        got.append((ds_d, pw, pb))
    assert all(torch.equal(u, v_) for u, v_ in zip(got[0], got[1]))
    ds_g = got[0][0].double().cpu().numpy()
    decided = np.abs(arg) > 4 * R.E * T
    bnd = e_dp[:, None] * np.abs(w64)[None, :] + R.E * np.abs(rds) + R.bound_store(rds, bf)
    err = np.abs(ds_g[:, :Fp] - rds)
    print(f"AGK dsum: max err {float(err[decided].max()) if decided.any() else 0.0:.3e}, undecided ReLU sides {int((~decided[:, :F]).sum())}")
    assert np.all(err[decided] <= bnd[decided]) and np.all(ds_g[:, F:Fp] == 0.0) and np.all(ds_g[:, Fp:] == SENT)
    e_s = 4 * R.E * T
    _close(got[0][1].double().sum(0).cpu().numpy(), rdw, (M + nb2) * R.E * np.abs(rdp[:, None] * s).sum(0) + (e_dp[:, None] * np.abs(s) + np.abs(rdp)[:, None] * e_s).sum(0) + 1e-30, "dw_psi")
    assert bool((got[0][1][:, F:] == 0).all())
    _close(float(got[0][2].double().sum()), rdb, (M + nb2) * R.E * np.abs(rdp).sum() + e_dp.sum() + 1e-30, "db_psi")


def test_attention_gate_entry_points_refuse():
    """-1 for a null argument, -2 for an unsupported geometry, like the neighbouring entry points; nothing is written."""
    lib = _lib()
    t = torch.zeros(64, 16, device=dev)
    v = torch.full((64,), SENT, device=dev)
    z = C.c_void_p(0)
    assert lib.pn2_ag_psi_fwd(0, z, 16, z, z, P(t), 16, z, z, P(t), 12, 16, 64, P(v), z, z, z) == -1
    assert lib.pn2_ag_psi_fwd(0, P(t), 16, z, z, P(t), 16, z, z, P(t), 12, 12, 64, P(v), z, z, z) == -2          # width not padded to 8
    assert lib.pn2_ag_psi_fwd(0, P(t), 18, z, z, P(t), 16, z, z, P(t), 12, 16, 64, P(v), z, z, z) == -2          # rows not 16-byte aligned
    assert lib.pn2_ag_psi_fwd(0, P(t), 512, z, z, P(t), 512, z, z, P(t), 300, 512, 2, P(v), z, z, z) == -2       # above 64 vectors
    assert lib.pn2_ag_apply_fwd(0, P(t), 16, P(t), 16, P(v), z, P(v), P(t), 16, 64, 12, 16, z) == -1
    assert lib.pn2_ag_apply_fwd(1, P(t), 16, P(t), 12, P(v), P(v), P(v), P(t), 16, 64, 12, 16, z) == -2
    assert lib.pn2_ag_blocks(0, 0, 16, 0) == -2 and lib.pn2_ag_blocks(0, 64, 12, 0) == -2 and lib.pn2_ag_blocks(0, 64, 16, 3) == -2
    torch.cuda.synchronize()
    assert bool((v == SENT).all()) and bool((t == 0).all())
