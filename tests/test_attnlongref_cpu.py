"""tests/attnlongref.py (the chunked recurrence the streamed attention kernels implement) against plain softmax(Q K^T) V and its autograd gradients,
float64, on the rows built to break a streaming softmax, at several chunk sizes including Nkv not a multiple of the chunk."""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import attnlongref as A  # noqa: E402

HD, HEADS, B, NQ = 32, 2, 1, 37


def _split(q, kv, heads, hd):
    Bq, Nq, Nkv = q.shape[0], q.shape[1], kv.shape[1]
    qq = q.double().reshape(Bq, Nq, heads, hd).transpose(1, 2)
    kk = kv.double().reshape(Bq, Nkv, 2, heads, hd).permute(2, 0, 3, 1, 4)
    return qq.contiguous(), kk[0].contiguous(), kk[1].contiguous()


def _plain(q, k, v, scale):
    s = (q @ k.transpose(-2, -1)) * scale
    return s.softmax(-1) @ v, torch.logsumexp(s, -1), s


def _check(q, k, v, chunk):
    scale = HD ** -0.5
    q, k, v = q.requires_grad_(True), k.requires_grad_(True), v.requires_grad_(True)
    ref, lse_ref, _ = _plain(q, k, v, scale)
    do = torch.randn(ref.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    ref.backward(do)
    with torch.no_grad():
        out, lse, visited = A.forward(q, k, v, scale, chunk)
        dq, dk, dv = A.backward(q, k, v, do, out, lse, scale, chunk)
    assert visited == math.ceil(k.shape[-2] / chunk)                  # the empty chunk behind the tail is never entered
    assert torch.isfinite(out).all() and torch.isfinite(lse).all()
    for got, want in ((out, ref), (lse, lse_ref), (dq, q.grad), (dk, k.grad), (dv, v.grad)):
        # float64 rounding only.  The absolute term covers the one-hot rows, whose dq is the cancelled sum of Nkv terms of size |dS| |k| <= ~100:
        # 1.1e-16 x 600 x 100 = 7e-12
        assert float((got - want).abs().max()) <= 1e-11 * float(want.abs().max()) + 1e-11


@pytest.mark.parametrize("chunk", [1, 7, 64, 128, 256, 600, 1000])
@pytest.mark.parametrize("kind", A.ADVERSARIAL)
def test_chunked_recurrence_on_adversarial_rows(kind, chunk):
    for Nkv in (600, 513, 257, 128, 5):
        g = torch.Generator().manual_seed(Nkv + chunk)
        q, kv = A.adversarial(kind, B, HEADS, NQ, Nkv, HD, 128, g)
        _check(*_split(q, kv, HEADS, HD), chunk)


def test_adversarial_rows_have_the_property_they_are_named_for():
    chunk, Nkv = 128, 600
    scale = HD ** -0.5
    rows = {}
    for kind in A.ADVERSARIAL:
        q, kv = A.adversarial(kind, B, HEADS, NQ, 513 if kind == "one_key_tail" else Nkv, HD, chunk, torch.Generator().manual_seed(3))
        qq, k, v = _split(q, kv, HEADS, HD)
        rows[kind] = (_plain(qq, k, v, scale)[2], k)
    s, k = rows["max_last"]
    assert float((s.argmax(-1) >= 512).double().mean()) > 0.9 and float(k[..., 512:, :].norm(dim=-1).mean()) > 2 * float(k[..., :128, :].norm(dim=-1).mean())
    s, _ = rows["max_first_rest_underflow"]
    assert bool((s.argmax(-1) < 5).all())
    assert float(torch.exp((s[..., 128:] - s.max(-1, keepdim=True).values).float()).max()) == 0.0          # fp32 exp of every later chunk is 0
    s, _ = rows["max_rises"]
    cm = torch.stack([s[..., c:c + chunk].max(-1).values for c in range(0, Nkv, chunk)], -1)
    assert bool((cm[..., 1:] > cm[..., :-1]).all())
    s, _ = rows["one_key_tail"]
    assert s.shape[-1] == 4 * chunk + 1 and bool((s.argmax(-1) == 4 * chunk).all())


def test_masked_tail_and_first_chunk_factor():
    """Two keys, chunk 4: the NaN padding rows must not reach the result; one key: softmax is 1, out = v, lse = the score."""
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(1, 1, 3, HD, generator=g, dtype=torch.float64) for _ in range(3))
    out, lse, visited = A.forward(q, k[..., :2, :], v[..., :2, :], 0.3, 4)
    ref, lref, _ = _plain(q, k[..., :2, :], v[..., :2, :], 0.3)
    assert visited == 1 and torch.allclose(out, ref, rtol=1e-13, atol=0) and torch.allclose(lse, lref, rtol=1e-13, atol=1e-15)
    out, lse, visited = A.forward(q, k[..., :1, :], v[..., :1, :], 0.3, 4)
    assert visited == 1 and torch.equal(out, v[..., :1, :].expand_as(out)) and torch.allclose(lse, (q @ k[..., :1, :].transpose(-2, -1))[..., 0] * 0.3, rtol=1e-13)
