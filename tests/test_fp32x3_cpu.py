"""fp32x3 mode without a GPU: the header code and the binding, the mode name, the dtype code at the C ABI boundary, and the float64 model of the kernels'
arithmetic (tests/fp32x3ref.py): the three-term bf16 split is exact, the six-product contraction stays within the gates, and the rms gate of the GPU
tests is at least 10 x tighter than the error of bf16 operands and 4 x tighter than that of a two-term split - a kernel that dropped the lo terms
could not pass."""
import os, re, sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
os.environ.setdefault("PN2_NO_PRETRAINED", "1")
import fp32ref as R  # noqa: E402
import fp32x3ref as X  # noqa: E402


def test_header_code_matches_binding():
    from pn2 import capi
    src = open(os.path.join(ROOT, "include", "pn2.h")).read()
    codes = dict(re.findall(r"#define\s+PN2_(F32X3)\s+(\d+)", src))
    assert int(codes["F32X3"]) == capi.F32X3 == 3
    assert len({capi.F32, capi.BF16, capi.F32F, capi.F32X3}) == 4


def test_mode_name_round_trips():
    import pn2
    from pn2 import capi, graph
    was = graph.get_compute_dtype()
    try:
        for name in ("fp32x3", "FP32X3", "f32x3"):
            pn2.set_compute_dtype(name)
            assert graph.get_compute_mode() == "fp32x3" and pn2.get_compute_dtype() == capi.F32X3
            pn2.set_compute_dtype(graph.get_compute_mode())
            assert pn2.get_compute_dtype() == capi.F32X3
    finally:
        pn2.set_compute_dtype(was)


def test_call_passes_code_3_through(monkeypatch):
    import pn2
    from pn2 import capi, graph
    lib = capi.load()
    seen = []
    names = ("pn2_conv_gemm", "pn2_conv_wgrad", "pn2_conv_gemm_tile", "pn2_pack_weight")
    for n in names:
        monkeypatch.setattr(lib, n, lambda *a, _n=n: seen.append((_n, a)) or 0)
    was = graph.get_compute_dtype()
    try:
        for mode in ("bf16", "fp32", "fp32fast", "fp32x3"):
            pn2.set_compute_dtype(mode)
            for n in names:
                capi.call.__dict__.pop(n, None)          # (checked wrappers are cached on the caller)
                seen.clear()
                getattr(capi.call, n)(capi.F32X3, 11, 22)
                assert seen == [(n, (capi.F32X3, 11, 22))], (mode, n, seen)
    finally:
        for n in names:
            capi.call.__dict__.pop(n, None)
        pn2.set_compute_dtype(was)


def test_tuner_key_suffix_is_its_own():
    from pn2 import capi, ops_conv
    assert ops_conv._MMA_KEY[capi.F32X3] == "f32x3" and ops_conv._MMA_KEY[capi.F32F] == "f32f"


def _wide_fp32(n, seed):
    g = torch.Generator().manual_seed(seed)
    mant = 1 + torch.rand(n, generator=g, dtype=torch.float64)
    e = torch.randint(-100, 101, (n,), generator=g).double()
    s = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    x = (s * mant * torch.exp2(e)).float()
    return torch.cat([x, torch.tensor([0.0, -0.0, 1.0, -1.0, 2.0 ** -100, -(2.0 ** 100), 3.0e38, -3.0e38])])


def test_split_is_exact_over_a_wide_range():
    x = _wide_fp32(200_000, 1)
    h, m, l = X.split3(x)
    assert bool((h.double() + m.double() + l.double() == x.double()).all())
    nz = x != 0
    assert bool((m[nz].abs().double() <= 2.0 ** -8 * x[nz].abs().double() * (1 + 2.0 ** -8)).all())
    assert bool((l[nz].abs().double() <= 2.0 ** -16 * x[nz].abs().double() * (1 + 2.0 ** -7)).all())
    # each term is a bf16 value
    for t in (h, m, l):
        assert bool((t.bfloat16().float() == t).all())
    # signed zeros stay zeros
    z = torch.tensor([0.0, -0.0])
    assert all(bool((t == 0).all()) for t in X.split3(z))


def test_split_edge_cases_match_the_header():
    h, m, l = X.split3(torch.tensor([float("nan"), float("inf"), -float("inf"), 3.40e38, -3.40e38]))
    tot = h.double() + m.double() + l.double()
    assert bool(torch.isnan(tot).all()), tot          # NaN stays NaN; inf and |x| above the largest bf16 (h rounds to inf) give NaN


@pytest.mark.parametrize("K", [72, 936, 1872, 6400])
def test_six_product_model_within_gates_and_canaries(K):
    g = torch.Generator().manual_seed(K)
    a = torch.randn(96, K, generator=g).double()
    b = (torch.randn(40, K, generator=g) * (2.0 / K) ** 0.5).double()
    a, b = a.float().double(), b.float().double()
    r = a @ b.t()
    S = a.abs() @ b.abs().t()
    got6 = X.x3_contract(a, b, 6)
    got2 = X.x3_contract(a, b, 3)
    ref32 = (a.float() @ b.float().t()).double()
    # the exact six-product sum (no in-chain rounding) is inside the worst case with the whole rounding budget left
    assert bool(((got6 - r).abs() <= 2.1 * R.U32 * S).all())
    assert bool(((got6 - r).abs() <= X.gate_fp32x3(S, K)).all())
    # the fp32 sum of the six-product chunks (16 k-values, round to nearest), as the kernel adds them, passes the worst case and the rms gate
    ha, ma, la = (t.double() for t in X.split3(a.float()))
    hb, mb, lb = (t.double() for t in X.split3(b.float()))
    acc = torch.zeros_like(r).float()
    for k0 in range(0, K, 16):
        sl = slice(k0, min(K, k0 + 16))
        c = (ha[:, sl] @ hb[:, sl].t() + ma[:, sl] @ mb[:, sl].t()) + (ha[:, sl] @ mb[:, sl].t() + ma[:, sl] @ hb[:, sl].t()) \
            + (ha[:, sl] @ lb[:, sl].t() + la[:, sl] @ hb[:, sl].t())
        acc = acc + c.float()
    emu = acc.double()
    assert bool(((emu - r).abs() <= X.gate_fp32x3(S, K) + 0.5 * R.spacing32(emu)).all())
    own = R.rms(ref32 - r)
    assert R.rms(emu - r) <= 2 * own, (R.rms(emu - r), own)
    # canaries: the rms gate of the GPU tests (2 x the reference's own fp32 error) is >= 10 x tighter than the error of bf16 operands.  A two-term split
    # (hh + hm + mh) errs by ~2^-16 per product, only ~16 x the fp32 error: no gate with room for fp32 rounding can be 10 x below it, but the rms gate
    # is >= 4 x below it - a kernel that dropped the lo terms fails by that margin
    two = R.rms(got2 - r)
    print(f"K {K}: rms error / reference fp32 error: six-product {R.rms(emu - r) / own:.3f}, two-term {two / own:.1f}")
    assert 10 * 2 * own <= R.bf16_error(a, b)
    assert 4 * 2 * own <= two, (own, two)


def test_wgrad_gate_covers_the_stage_chain():
    g = torch.Generator().manual_seed(5)
    M, C, K = 1000, 24, 40
    dy = torch.randn(M, C, generator=g).double()
    x = torch.randn(M, K, generator=g).double()
    r = dy.t() @ x
    S = dy.abs().t() @ x.abs()
    got = X.x3_contract(dy.t().contiguous(), x.t().contiguous(), 6)
    slabs = got[None]
    assert bool(((got - r).abs() <= X.wgrad_tol_x3(got, slabs, 1, S, M)).all())
