"""CPU pins of the reference helpers of the fp32 / fp32fast conv kernel tests (tests/fp32ref.py) against torch's own conv in float64, the precision gates'
canary, and the consistency of the shipped fp32fast tuning entries."""
import json
import os, sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fp32ref as R  # noqa: E402

TABLE_PATH = os.path.join(os.path.dirname(HERE), "pranet-v2_amd", "pn2", "tuned_gfx950.json")

# N, H, W, Cin, Cout, KH, KW, stride, pad_h, pad_w, dil_h, dil_w
SMALL = [
    (2, 7, 9, 8, 16, 1, 1, 1, 0, 0, 1, 1),
    (2, 7, 9, 8, 16, 3, 3, 1, 1, 1, 1, 1),
    (1, 10, 11, 16, 8, 3, 3, 2, 1, 1, 1, 1),
    (2, 9, 8, 8, 8, 3, 3, 1, 3, 3, 3, 3),
    (1, 8, 12, 8, 24, 1, 5, 1, 0, 2, 1, 1),
    (1, 12, 8, 8, 8, 7, 1, 1, 3, 0, 1, 1),
    (1, 13, 13, 8, 8, 3, 3, 2, 2, 2, 2, 2),
    (2, 16, 16, 8, 8, 4, 4, 4, 0, 0, 1, 1),
]


def _packed_fwd(w):          # wp[co][tap*Cin + ci]
    Cout, Cin, KH, KW = w.shape
    return w.permute(0, 2, 3, 1).reshape(Cout, KH * KW * Cin)


def _packed_dgrad(w):        # wp[ci][tap*Cout + co]
    Cout, Cin, KH, KW = w.shape
    return w.permute(1, 2, 3, 0).reshape(Cin, KH * KW * Cout)


@pytest.mark.parametrize("geom", SMALL)
def test_gather_helpers_match_torch_conv(geom):
    N, H, W, Cin, Cout, KH, KW, s, ph, pw, dh, dw = geom
    OH = (H + 2 * ph - dh * (KH - 1) - 1) // s + 1
    OW = (W + 2 * pw - dw * (KW - 1) - 1) // s + 1
    g = torch.Generator().manual_seed(sum(geom))
    x = torch.randn(N, H, W, Cin, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, KH, KW, generator=g, dtype=torch.float64)
    dy = torch.randn(N, OH, OW, Cout, generator=g, dtype=torch.float64)
    # forward: rows of the gathered operand against the packed weight
    ref = F.conv2d(x.permute(0, 3, 1, 2), w, None, s, (ph, pw), (dh, dw)).permute(0, 2, 3, 1).reshape(-1, Cout)
    rows = torch.arange(N * OH * OW)
    # channel slice of a wider buffer: the helper must read channels [0, Cin) only
    xw = torch.cat([x, torch.full((N, H, W, 8), float("nan"), dtype=torch.float64)], -1).reshape(-1, Cin + 8)
    got = R.gather(xw, rows, (N, H, W, OH, OW, Cin, KH, KW, s, ph, pw, dh, dw), False) @ _packed_fwd(w).t()
    assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12)
    # dgrad: the transposed gather in desc terms (gathered dy [N, OH, OW], produced dx [N, H, W])
    op = (H - ((OH - 1) * s - 2 * ph + dh * (KH - 1) + 1), W - ((OW - 1) * s - 2 * pw + dw * (KW - 1) + 1))
    refd = F.conv_transpose2d(dy.permute(0, 3, 1, 2), w, None, s, (ph, pw), op, 1, (dh, dw)).permute(0, 2, 3, 1).reshape(-1, Cin)
    sub = R.sample_rows(N * H * W, 5, block=16, edge=4)
    gotd = R.gather(dy.reshape(-1, Cout), sub, (N, OH, OW, H, W, Cout, KH, KW, s, ph, pw, dh, dw), True) @ _packed_dgrad(w).t()
    assert torch.allclose(gotd, refd[sub], rtol=1e-12, atol=1e-12)
    # weight gradient rows (chunked over pixels) against autograd
    wr = torch.zeros_like(w, requires_grad=True)
    F.conv2d(x.permute(0, 3, 1, 2), wr, None, s, (ph, pw), (dh, dw)).backward(dy.permute(0, 3, 1, 2))
    co = [0, Cout - 1]
    gw, S = R.wgrad_rows(dy.reshape(-1, Cout), x.reshape(-1, Cin), co, (N, H, W, OH, OW, Cin, KH, KW, s, ph, pw, dh, dw), chunk=37)
    assert torch.allclose(gw, _packed_fwd(wr.grad)[co], rtol=1e-12, atol=1e-12)
    wa = torch.zeros_like(w, requires_grad=True)
    F.conv2d(x.abs().permute(0, 3, 1, 2), wa, None, s, (ph, pw), (dh, dw)).backward(dy.abs().permute(0, 3, 1, 2))
    assert torch.allclose(S, _packed_fwd(wa.grad)[co], rtol=1e-12, atol=1e-12)


def test_sample_rows_cover_every_tile_pair():
    for M in (1, 63, 64, 200, 991232):
        rows = R.sample_rows(M, 3)
        assert int(rows.min()) == 0 and int(rows.max()) == M - 1 and bool((rows[1:] > rows[:-1]).all())
        blocks = torch.unique(rows // 64)
        assert blocks.numel() == (M + 63) // 64


def test_spacing32():
    v = torch.tensor([1.0, -1.0, 3.0, 2.0 ** -10, 0.0], dtype=torch.float64)
    sp = R.spacing32(v)
    assert sp[0] == 2.0 ** -23 and sp[1] == 2.0 ** -23 and sp[2] == 2.0 ** -22 and sp[3] == 2.0 ** -33 and 0 < sp[4] < 1e-44


@pytest.mark.parametrize("K", [8, 32, 72, 288, 1152, 9216])
def test_gates_are_ten_times_tighter_than_bf16_operands(K):
    """Canary: a gate that is not at least 10 x tighter than the error of bf16-rounded operands could not tell an fp32 kernel from one that drops operand
    bits.  fp32: the correct-rounding gate; fp32fast: the statistical gate (2 x the reference's own fp32 rms error).  The elementwise worst-case bound of
    fp32fast grows like K / 16 while the bf16 error grows like sqrt(K): it is a safety net for gross errors, and held to the canary only for K <= 288."""
    g = torch.Generator().manual_seed(K)
    a = torch.randn(256, K, generator=g).double()
    b = torch.randn(64, K, generator=g).double()
    r = a @ b.t()
    S = a.abs() @ b.abs().t()
    ebf = R.bf16_error(a, b)
    got32 = r.float().double()
    assert R.rms(R.gate_fp32(got32, r, S, K)) * 10 <= ebf
    ref32 = (a.float() @ b.float().t()).double()
    assert 2 * R.rms(ref32 - r) * 10 <= ebf
    if K <= 288:
        assert R.rms(R.gate_fp32fast(S, K)) * 10 <= ebf
    # and the fp32 gate catches a double accumulator rounded to fp32 after every 32-wide K-step
    acc = torch.zeros_like(r)
    for k0 in range(0, K, 32):
        acc = (acc + a[:, k0:k0 + 32] @ b[:, k0:k0 + 32].t()).float().double()
    if K > 32:
        assert bool(((acc - r).abs() > R.gate_fp32(acc, r, S, K)).any())


def test_shipped_fp32fast_entries_parse_to_valid_codes():
    """Every fp32fast entry of the shipped table is a code the library takes: forward / dgrad codes with kernel bits 1 (register-staged), BM in {64, 128},
    BN in {32, 64}; weight gradients (kernel 1, splits >= 1); keys well formed."""
    table = R.table_codes(json.load(open(TABLE_PATH)))
    assert len(table) >= 200
    ids = set()
    for key, v in table.items():
        ids.add(R.key_id(key))
        if key[0] == "g":
            assert isinstance(v, int) and len(key) in (18, 23, 24), key
            assert v & 3 == 1 and (v >> 2) & 3 in (1, 2) and (v >> 4) & 3 in (1, 2) and v >> 6 == 0, (key, v)
            if "ep" in key:
                assert key[16] == 1 and key[17] == "ep" and (key[22] == "f32f" or key[22:] == ("pool", "f32f")), key
        else:
            assert key[0] == "w" and len(key) == 19, key
            kern, ns = v
            assert kern == 1 and ns >= 1, (key, v)
    assert len(ids) == len(table), "test ids of the shipped fp32fast entries are not unique"
