"""tests/vitref.py without a GPU: every reference is held to torch in float64 (F.layer_norm, F.conv2d(groups=C), F.gelu, autograd for all gradients), the
mirror of the launch geometry is held to the library wherever the library exposes the plan (host-only exports and refusal codes), every kernel route that
tests/test_gpu_vit_kernels.py means to reach is shown to be reached by a case of the tables, and the fp32 evaluation of each reference is shown to pass the
bound the kernel gets (lines starting with VITC, run with -s).  If a threshold of a plan moves, the route assertions say which case fell off its route."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import vitref as R

F64, F32 = torch.float64, torch.float32
PTR = C.c_void_p(4096)          # a non-null pointer for calls that are refused before anything reads it
needs_clean_env = pytest.mark.skipif(not R.env_clean(), reason="PN2_DW_WIN / PN2_DW_SEG change the depth-wise plans the mirror describes")


def _lib():
    from pn2 import capi
    return capi, capi.load()


def close(a, b, rtol=1e-12):
    return bool(((a - b).abs() <= rtol * (1 + b.abs().max())).all())


# ================================================================================================================ references against torch
@pytest.mark.parametrize("case", [c for c in R.ln_cases() if c[2] <= 64], ids=R.ln_id)
def test_layernorm_refs_equal_torch(case):
    dt, Cc, M, form, eps, content = case
    inp = R.ln_inputs(case)
    e = R.f32(eps)
    x = inp["x"].clone().requires_grad_(True)
    g, b = inp["gamma"].clone().requires_grad_(True), inp["beta"].clone().requires_grad_(True)
    y = F.layer_norm(x, (Cc,), g, b, e)
    y.backward(inp["dy"])
    y64, mean, rstd = R.ln_fwd_ref(inp["x"], inp["gamma"], inp["beta"], e)
    # torch's own float64 statistics lose (mean / spread)^2 = 1e10 of their 2^-53 on the rows with mean >> spread
    tol = 1e-5 if content else 1e-11
    assert close(y64, y.detach(), tol) and close(mean, inp["x"].mean(1)) and close(rstd, 1 / torch.sqrt(inp["x"].var(1, unbiased=False) + e), tol)
    dx, dg, db = R.ln_bwd_ref(inp["dy"], inp["x"], inp["gamma"], mean, rstd)
    assert close(dx, x.grad, tol) and close(dg, g.grad, tol) and close(db, b.grad)
    kinds = R.ln_row_kinds(M, content)
    for r, k in enumerate(kinds):
        if k == "const":          # y = beta, rstd = eps^-1/2
            assert torch.equal(y64[r], inp["beta"]) and abs(float(rstd[r]) - e ** -0.5) <= 1e-12 * e ** -0.5
        if k == "bigmean" and dt == "fp32":        # a one-pass variance E[x^2] - mean^2 in fp32 goes negative or loses every digit on these rows
            x32 = inp["x"][r].to(F32)
            one_pass = float((x32 * x32).mean() - x32.mean() ** 2)
            true = float(inp["x"][r].var(unbiased=False))
            assert one_pass < 0 or abs(one_pass - true) > 0.05 * true, (one_pass, true)
    if content:
        assert set(kinds) == set(R.ROW_KINDS)
    assert bool((inp["gamma"] == 0).any()) and (Cc < 8 or bool((inp["gamma"] < 0).any()))


@pytest.mark.parametrize("shape", R.DW_SHAPES, ids=str)
def test_depthwise_refs_equal_torch(shape):
    """flip = 0 is F.conv2d(groups=C); flip = 1 is its data gradient; the weight / bias gradients are autograd's; GELU and its derivative are F.gelu's."""
    N, H, W, Cc = shape
    inp = R.dw_inputs(shape, "bf16")
    x = inp["x"].permute(0, 3, 1, 2).clone().requires_grad_(True)
    w, b = inp["w"].reshape(Cc, 1, 3, 3).clone().requires_grad_(True), inp["b"].clone().requires_grad_(True)
    z = F.conv2d(x, w, b, padding=1, groups=Cc)
    z.backward(inp["dy"].permute(0, 3, 1, 2))
    assert close(R.dwconv_ref(inp["x"], inp["w"], inp["b"]), z.detach().permute(0, 2, 3, 1))
    assert close(R.dwconv_ref(inp["x"], inp["w"]) + inp["old"], R.dwconv_ref(inp["x"], inp["w"], None, 0, inp["old"]))
    assert close(R.dwconv_ref(inp["dy"], inp["w"], None, 1), x.grad.permute(0, 2, 3, 1))
    gw, gb = R.dw_wgrad_ref(inp["dy"], inp["x"])
    assert close(gw, w.grad.reshape(Cc, 9)) and close(gb, b.grad)
    zp = inp["zpre"].clone().requires_grad_(True)
    y = F.gelu(zp)
    y.backward(torch.ones_like(y))
    assert close(R.gelu_ref(inp["zpre"]), y.detach()) and close(R.gelu_grad_ref(inp["zpre"]), zp.grad)


def test_colsum_and_scale_refs_equal_torch():
    x = R.values("cs", (37, 24), "bf16")
    assert close(R.colsum_ref(x), torch.einsum("mc->c", x))
    s, res = torch.tensor(R.SCALES, dtype=F32).to(F64), R.values("res", (3, 24), "bf16")
    xs = R.values("sc", (3, 24), "bf16")
    assert torch.equal(R.scale_ref(xs, s), torch.stack([xs[n] * s[n] for n in range(3)]))
    assert torch.equal(R.scale_ref(xs, s, res), R.scale_ref(xs, s) + res) and bool((R.scale_ref(xs, s)[0] == 0).all())


def test_gelu_grids_hold_what_they_promise():
    z = R.gelu_grid("fp32")
    assert z.numel() == 204800 and R.representable(z, "fp32") and 190000 < int(((z >= -9) & (z <= 9)).sum())
    z32 = z.to(F32)
    for v in (R.SWITCH, R.CLAMP):
        for s in (1.0, -1.0):
            c = torch.tensor(s * v, dtype=F32)
            for nb in (c, torch.nextafter(c, torch.tensor(9e9)), torch.nextafter(c, torch.tensor(-9e9))):
                assert bool((z32 == nb).any())
    # both pieces of the erf are entered on both sides of the switch: |z / sqrt 2| <= and > 0.921875 in the kernel's own fp32 product
    a = (z32 * torch.tensor(0.70710678118654752, dtype=F32)).abs()
    assert bool((a <= 0.921875).any()) and bool((a > 0.921875).any()) and bool((a > 4).any())
    for v in (0.0, 1e-20, 30.0):
        assert bool((z32 == torch.tensor(v, dtype=F32)).any()) and bool((z32 == torch.tensor(-v, dtype=F32)).any())
    assert bool(torch.signbit(z32[z32 == 0]).any()) and not bool(torch.signbit(z32[z32 == 0]).all())
    zb = R.gelu_grid("bf16")
    assert zb.numel() % 8 == 0 and R.representable(zb, "bf16") and float(zb.abs().max()) == 16.0
    assert zb.unique().numel() == 2 * (0x4180 + 1) - 1          # every bf16 from 0 to 16 with both signs (+-0 are one value)


# ================================================================================================================ the mirror against the library
def test_layernorm_and_rows_plans_equal_library():
    capi, lib = _lib()
    for dt in R.VEC:
        widths = set(R.LN_WIDTHS[dt]) | set(R.LN_REFUSED[dt]) | set(range(2, 2200, 2))
        for Cc in sorted(widths):
            assert lib.pn2_ln_slots(R.DT[dt], Cc) == R.ln_slots(dt, Cc), (dt, Cc)
    for M in sorted({c[2] for c in R.ln_cases()} | {c[2] for c in R.colsum_cases()} | {1, 511, 512, 513, 2048, 2049, 1 << 20}):
        for unit in (1, 2, 4, 8, 16, 32, 64, 128, 256):
            assert lib.pn2_rows_blocks(M, unit) == R.rows_blocks(M, unit), (M, unit)


def test_layernorm_refusals():
    """A width that is no multiple of the vector, or one vector above the widest, is refused with -2 before any launch, forward and backward."""
    capi, lib = _lib()
    for dt in R.VEC:
        V = R.VEC[dt]
        assert R.LN_REFUSED[dt][0] % V and R.LN_REFUSED[dt][1] == R.LN_MAXC[dt] + V
        assert R.ln_lpr(dt, R.LN_MAXC[dt]) == 64 and R.LN_MAXC[dt] in R.LN_WIDTHS[dt]
        for Cc in R.LN_REFUSED[dt]:
            assert R.ln_lpr(dt, Cc) == -1
            assert lib.pn2_layernorm_fwd(R.DT[dt], PTR, Cc, PTR, Cc, 5, Cc, PTR, PTR, 1e-5, PTR, PTR, None) == -2
            assert lib.pn2_layernorm_bwd(R.DT[dt], PTR, Cc, PTR, Cc, 5, Cc, PTR, PTR, PTR, PTR, Cc, 0, PTR, PTR, 1, None) == -2
        Cc = R.LN_WIDTHS[dt][2]          # a block count other than pn2_rows_blocks is refused too
        assert lib.pn2_layernorm_bwd(R.DT[dt], PTR, Cc, PTR, Cc, 5000, Cc, PTR, PTR, PTR, PTR, Cc, 0, PTR, PTR, 1, None) == -2


def test_colsum_plans_equal_library():
    capi, lib = _lib()
    for dt, Cc, M, ld in R.colsum_cases() + [("bf16", 12, 5, 12), ("fp32", 8, 5, 10), ("bf16", 64, 4096, 64), ("fp32", 2048, 123904, 2048)]:
        j = capi.ColsumInJob()
        j.dy, j.partial, j.M, j.C, j.ld = PTR, PTR, M, Cc, ld
        got = lib.pn2_colsum_job_blocks(R.DT[dt], C.byref(j))
        plan = R.colsum_plan(dt, M, Cc, ld)
        if plan is None:
            assert got == -2, (dt, Cc, M, ld)
            continue
        assert (j.cvp, j.rows, got) == plan, (dt, Cc, M, ld)
        assert lib.pn2_colsum_unit(R.DT[dt], Cc) == 256 // plan[0] and lib.pn2_rows_blocks(M, 256 // plan[0]) == plan[2]
        assert lib.pn2_colsum(R.DT[dt], PTR, ld, M, Cc, PTR, plan[2] + 1, None) == -2
    for Cc in R.FIN_C:
        assert lib.pn2_colsum_finalize_blocks(Cc) == (Cc + 31) // 32


@needs_clean_env
def test_depthwise_plans_equal_library():
    capi, lib = _lib()
    shapes = list(R.DW_SHAPES) + list(R.DW_LARGE.values()) + [(n, h, h, c) for n in (1, 16) for h in (1, 11, 16, 88, 128) for c in (2, 6, 8, 64, 66, 320, 512)]
    for dt in R.VEC:
        for N, H, W, Cc in shapes:
            assert lib.pn2_dwconv3x3_colsum_blocks(R.DT[dt], N, H, W, Cc) == R.dw_colsum_blocks(dt, N, H, W, Cc), (dt, N, H, W, Cc)
            assert lib.pn2_dwconv3x3_wgrad_blocks(R.DT[dt], N, H, W, Cc) == R.dw_wgrad_plan(dt, N, H, W, Cc)["nchunk"], (dt, N, H, W, Cc)
        assert lib.pn2_dwconv3x3(R.DT[dt], PTR, PTR, PTR, PTR, None, 2, 3, 3, 5, 0, 0, None) == -2          # odd channel count
        assert lib.pn2_dwconv3x3_wgrad(R.DT[dt], PTR, PTR, PTR, 99999, 2, 3, 3, 8, None, None, None) == -2  # a chunk count other than _wgrad_blocks
    assert lib.pn2_dwconv3x3_colsum(R.DT["bf16"], PTR, PTR, PTR, PTR, 2, 3, 3, 8, 0, PTR, 99999, None) == -2
    assert lib.pn2_dwconv3x3_colsum(R.DT["fp32"], PTR, PTR, PTR, PTR, 2, 3, 3, 8, 0, PTR, 1, None) == -2      # column sums only ride on the window kernels
    assert lib.pn2_gelu_bwd(R.DT["bf16"], PTR, PTR, PTR, 12, None) == -2 and lib.pn2_scale_samples(R.DT["fp32"], PTR, PTR, PTR, None, 3, 6, None) == -2


# ================================================================================================================ every route is reached
def test_layernorm_cases_reach_every_route():
    cases = R.ln_cases()
    assert {R.ln_lpr(c[0], c[1]) for c in cases} == {8, 16, 32, 64}
    for dt in R.VEC:
        mine = [c for c in cases if c[0] == dt]
        assert {R.ln_nv(dt, c[1]) for c in mine} == {1, R.LN_NV}, dt
        assert {R.ln_nv(dt, c[1]) for c in mine if c[5]} == {1, R.LN_NV}, dt          # row content on both instantiations
        assert {c[1] for c in mine} >= {R.VEC[dt], 32, 64, 160, 320, 512, R.LN_MAXC[dt]}
        assert {c[3] for c in mine} == set(R.LN_FORMS) and {c[4] for c in mine} == set(R.EPS)
        V = R.VEC[dt]
        for ld in R.ln_ld(dt, 64, "pad"):
            assert ld > 64 and ld % V == 0
        assert {(ld - 64) // V for ld in R.ln_ld(dt, 64, "pad")} == {1, 3}
        for Cc in R.LN_WIDTHS[dt]:
            rpb = R.ln_slots(dt, Cc)
            assert {c[2] for c in mine if c[1] == Cc and not c[5]} >= {1, rpb - 1, rpb + 1}
    assert R.ln_lpr("bf16", 520) == 64 and 520 // 8 - 64 == 1          # four-vector instantiation, one live lane in its second round
    trips = {}
    for dt, Cc, M in R.LN_LONG:
        nslot = R.ln_slots(dt, Cc)
        rows = R.rows_for(M, nslot)
        last = M - (R.rows_blocks(M, nslot) - 1) * rows
        assert rows % nslot == 0 and last % nslot != 0, (dt, Cc, M)          # the last iteration of the last workgroup is partly live
        trips.setdefault(rows // nslot, []).append((R.ln_nv(dt, Cc), R.ln_lpr(dt, Cc), last))
    assert set(trips) >= {2, 3}
    assert {t[0] for t in trips[2]} == {1, R.LN_NV} and {t[1] for t in trips[2]} >= {8, 64}
    assert any(t[2] == 1 for v in trips.values() for t in v)          # a last workgroup that holds a single row
    for c in cases:          # everything else runs the row loop exactly once
        if c[:3] not in R.LN_LONG:
            assert R.rows_for(c[2], R.ln_slots(c[0], c[1])) == R.ln_slots(c[0], c[1])


def test_colsum_cases_reach_every_route():
    seen = set()
    for dt, Cc, M, ld in R.colsum_cases():
        cvp, rows, nblk = R.colsum_plan(dt, M, Cc, ld)
        Rl, CV = 256 // cvp, Cc // R.VEC[dt]
        if M > 512 * Rl:
            assert rows > Rl and nblk > 1 and 0 < M - (nblk - 1) * rows < rows, (dt, Cc, M)          # rows walked more than once per lane, a short last block
            seen.add((dt, "long", CV > cvp))
        if CV > cvp:
            assert CV - cvp == 1          # the second pass of the channel loop has one live vector
            seen.add((dt, "pass2"))
        if CV == 1:
            assert Rl == 256
            seen.add((dt, "lanes256"))
        seen.add((dt, "ld>C" if ld > Cc else "ld=C"))
        if M == max(1, Rl - 1):
            seen.add((dt, "R-1"))
    for dt in R.VEC:
        assert {k[1] for k in seen if k[0] == dt} >= {"long", "pass2", "lanes256", "ld>C", "ld=C", "R-1"}, dt
    # finalize: the four-deep loop runs when some lane has r + 24 < nblk (nblk >= 25), the tail loop whenever nblk % 32 leaves rows over
    assert any(n >= 25 for n in R.FIN_NBLK) and any(n < 25 for n in R.FIN_NBLK) and any(n > 32 and n % 32 for n in R.FIN_NBLK)
    assert set(R.FIN_NBLK) >= {1, 7, 8, 9, 31, 32, 33, 57} and set(R.FIN_C) >= {1, 31, 33, 320}


@needs_clean_env
def test_depthwise_cases_reach_every_route():
    win_vt, row_vt, seg_ends, multi_group, seg32 = set(), set(), set(), False, False
    for dt in R.VEC:
        for shape in list(R.DW_SHAPES) + [R.DW_LARGE[dt]]:
            for flip, bias, gelu, acc in R.DW_COMBOS:
                p = R.dw_plan(dt, gelu, acc, *shape)
                assert shape[3] % p["VT"] == 0
                (win_vt if p["win"] else row_vt).add((dt, p["VT"]))
                if p["win"]:
                    W = shape[2]
                    seg_ends |= {(min(W, (s + 1) * p["SEG"]) - s * p["SEG"]) % 3 for s in range(p["SPR"])}
                    multi_group |= p["gy"] > 1 and p["CV"] % p["cvp"] == 1
                    seg32 |= p["seg32"] and p["SEG"] == 17
    assert win_vt == {("bf16", 4), ("bf16", 2)}
    assert row_vt >= {("bf16", 8), ("bf16", 4), ("bf16", 2), ("fp32", 4), ("fp32", 2)}
    assert seg_ends == {0, 1, 2} and multi_group and seg32
    big = R.dw_plan("bf16", False, True, *R.DW_LARGE["bf16"])
    assert not big["win"] and big["VT"] == 8                                     # accumulate = 1 leaves the window kernel for the 8-channel row walk
    assert R.dw_plan("fp32", False, False, *R.DW_LARGE["fp32"])["VT"] == 4       # the 4-channel fp32 row walk
    assert R.dw_plan("bf16", False, False, 2, 4, 17, 516)["gy"] == 2
    assert R.dw_plan("bf16", False, False, 3, 5, 9, 64)["SEG"] == 5 and R.dw_plan("bf16", False, False, 3, 5, 9, 64)["SPR"] == 2
    for s in R.DW_WALIGN_SHAPES:          # the 16-byte weight loads that walign switches exist only at 4 or 8 channels per thread
        assert R.dw_plan("bf16", False, False, *s)["VT"] == 4 and R.dw_plan("fp32", False, True, *s)["VT"] in (2, 4)
    # weight gradient: fewer segments than a chunk has lanes; a short last chunk; window kernels at 4 and 2 channels, row walks at 2
    plans = {(dt, s): R.dw_wgrad_plan(dt, *s) for dt in R.VEC for s in list(R.DW_SHAPES) + [R.DW_LARGE[dt]]}
    assert any(p["nseg"] < p["R"] for p in plans.values())
    assert any(p["nchunk"] > 1 and p["nseg"] % p["SPC"] for p in plans.values())
    assert {p["VT"] for k, p in plans.items() if p["win"]} == {4, 2} and {p["VT"] for k, p in plans.items() if not p["win"]} == {2}
    assert any(p["gy"] > 1 for p in plans.values())
    # DropPath / gelu_bwd: the capped grid takes a second trip, the small case is no multiple of a workgroup's vectors
    assert R.CAP_VECS > R.GRID_CAP * 256 and R.grid_for(R.CAP_VECS) == R.GRID_CAP and R.CAP_VECS % 3 == 0 and R.SCALE_VECS % 256


# ================================================================================================================ ref32 passes what the kernel has to pass
def _self_check(tag, dt, exp):
    return max(R.check(f"{tag} {name}", dt, r32.to(F64), r64, b, r32, prefix="VITC") for name, (r64, r32, b) in exp.items())


@pytest.mark.parametrize("case", R.ln_cases(), ids=R.ln_id)
def test_layernorm_ref32_inside_bounds(case):
    inp = R.ln_inputs(case)
    _self_check("ln_fwd " + R.ln_id(case), case[0], R.ln_fwd_expect(case, inp))
    for acc in (0, 1):
        _self_check(f"ln_bwd acc{acc} " + R.ln_id(case), case[0], R.ln_bwd_expect(case, inp, acc))


@pytest.mark.parametrize("case", R.colsum_cases(), ids=str)
def test_colsum_ref32_inside_bounds(case):
    dt, Cc, M, ld = case
    x = R.values("colsum", (M, Cc), dt)
    R.check(f"colsum {case}", dt, R.colsum_ref(x, F32).to(F64), R.colsum_ref(x), R.nterm_bound(M, x.abs().sum(0)), R.colsum_ref(x, F32), prefix="VITC")


@pytest.mark.parametrize("dt", list(R.VEC))
@pytest.mark.parametrize("shape", R.DW_SHAPES, ids=str)
def test_depthwise_ref32_inside_bounds(shape, dt):
    inp = R.dw_inputs(shape, dt)
    for flip, bias, gelu, acc in R.DW_COMBOS:
        _self_check(f"dw {shape} f{flip}b{bias}g{gelu}a{acc}", dt, R.dw_expect(inp, dt, flip, bias, gelu, acc))
    r64, r32, b = R.dz_expect(inp, dt)
    R.check(f"dz {shape}", dt, r32.to(F64), r64, b, r32, prefix="VITC")
    _self_check(f"wgrad {shape}", dt, R.wgrad_expect(inp["dy"], inp["x"]))


def test_gelu_ref32_inside_bounds():
    """The scale of the GELU bounds is measured here as it is in the GPU test: torch's fp32 GELU reaches `torch_share` of the bound's shape, the bound is three
    times that.  The reference's own formula in fp32 must pass it on both grids."""
    K = R.gelu_scales()
    print(f"\nVITC gelu torch fp32 shares {R._SCALES['torch_share']} -> K {K}")
    assert K[0] >= 3 and K[1] >= 3 and K[0] < 30 and K[1] < 30
    for dt in R.VEC:
        z = R.gelu_grid(dt)
        R.check("gelu grid", dt, R.gelu_ref(z, F32).to(F64), R.gelu_ref(z), R.gelu_bound(z), R.gelu_ref(z, F32), prefix="VITC")
        R.check("gelu' grid", dt, R.gelu_grad_ref(z, F32).to(F64), R.gelu_grad_ref(z), R.gelu_grad_bound(z), R.gelu_grad_ref(z, F32), prefix="VITC")


def test_scale_ref32_inside_bounds():
    for dt in R.VEC:
        n = R.SCALE_VECS * R.VEC[dt]
        x, res = R.values("scale_x", (3, n), dt), R.values("scale_r", (3, n), dt)
        s = torch.tensor(R.SCALES, dtype=F32).to(F64)
        assert n % (256 * R.VEC[dt]) and R.representable(s, "fp32") and float(s[0]) == 0
        for r in (None, res):
            R.check(f"scale res{r is not None}", dt, R.scale_ref(x, s, r, F32).to(F64), R.scale_ref(x, s, r), R.scale_bound(x, s, r, dt), R.scale_ref(x, s, r, F32), prefix="VITC")
        assert torch.equal(R.scale_ref(x, s, None, F32).to(F64), R.rt(R.scale_ref(x, s), "fp32"))
