"""float64 restatement of what the streamed attention kernels (csrc/pn2_attn.hip, pn2_attn_long_*) compute, and the rows built to break a streaming
softmax that the CPU and GPU tests share.  Not a test module.

Forward, per chunk of `chunk` keys with m / l / O the running maximum, sum and un-normalised output of a row:
    m' = max(m, max_j s_j)   a = exp(m - m') (0 for the first chunk)   l = l a + sum_j exp(s_j - m')   O = O a + exp(s - m') V
out = O / l, lse = m + log l.  Keys past Nkv in the last chunk are masked; a chunk without a valid key is never visited, so m' is always finite.
Backward, per key range from lse and delta = rowsum(dO * out):  P = exp(s - lse), dS = P (dP - delta), dQ += scale dS K (summed over the ranges),
dK = scale dS^T Q and dV = P^T dO of the range."""
import math

import torch


def forward(q, k, v, scale, chunk):
    """q [..., Nq, hd], k / v [..., Nkv, hd] float64 -> (out, lse, chunks visited).  The key axis is padded to whole chunks with NaN rows: a masked
    key must never reach a sum, and the all-padding chunk that a rounded-up loop bound would add must never be entered."""
    Nq, Nkv = q.shape[-2], k.shape[-2]
    pad = (-Nkv) % chunk + chunk                                      # the partial tail and one whole empty chunk behind it
    nan = lambda t: torch.cat([t, t.new_full(t.shape[:-2] + (pad, t.shape[-1]), float("nan"))], -2)
    kp, vp = nan(k), nan(v)
    m = q.new_full(q.shape[:-1], -math.inf)
    l = torch.zeros_like(m)
    o = torch.zeros_like(q)
    visited = 0
    for key0 in range(0, kp.shape[-2], chunk):
        if key0 >= Nkv:                                               # no valid key: not visited
            continue
        visited += 1
        valid = torch.arange(key0, key0 + chunk) < Nkv
        s = (q @ kp[..., key0:key0 + chunk, :].transpose(-2, -1)) * scale
        s = torch.where(valid, s, s.new_tensor(-math.inf))
        m2 = torch.maximum(m, s.max(-1).values)
        assert bool(torch.isfinite(m2).all())
        a = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - m2))          # first chunk: 0, not exp(-inf + inf)
        p = torch.exp(s - m2[..., None])                              # exp(-inf) = 0 for the masked tail
        l = l * a + p.sum(-1)
        vc = torch.where(valid[:, None], vp[..., key0:key0 + chunk, :], vp.new_zeros(()))
        o = o * a[..., None] + p @ vc
        m = m2
    return o / l[..., None], m + torch.log(l), visited


def backward(q, k, v, do, out, lse, scale, chunk):
    """(dq, dk, dv) by key ranges, the way the kernels walk them."""
    Nkv = k.shape[-2]
    delta = (do * out).sum(-1)
    dq = torch.zeros_like(q)
    dk, dv = torch.zeros_like(k), torch.zeros_like(v)
    for key0 in range(0, Nkv, chunk):
        kc, vc = k[..., key0:key0 + chunk, :], v[..., key0:key0 + chunk, :]
        p = torch.exp((q @ kc.transpose(-2, -1)) * scale - lse[..., None])
        ds = p * (do @ vc.transpose(-2, -1) - delta[..., None]) * scale
        dq = dq + ds @ kc
        dk[..., key0:key0 + chunk, :] = ds.transpose(-2, -1) @ q
        dv[..., key0:key0 + chunk, :] = p.transpose(-2, -1) @ do
    return dq, dk, dv


ADVERSARIAL = ("max_last", "max_first_rest_underflow", "max_rises", "one_key_tail")


def adversarial(kind, B, heads, Nq, Nkv, hd, chunk, gen):
    """(q [B][Nq][heads*hd], kv [B][Nkv][2*heads*hd]) fp32 with q scaled by 8.  Dimension 0 of every head carries the structure: q has a positive
    component there (>= 8 * 3 after the scaling) and key j the ramp r_j, so the score of key j is (q_0 r_j + noise) * scale.
      max_last                  r grows with the key index (and so do the key norms): the row maximum is in the last chunk
      max_first_rest_underflow  r = 0 on the first 5 keys, -40 from `chunk` on: later chunks are >= 8*3*40 / sqrt(hd) >= 120 below the maximum, exp -> 0 in fp32
      max_rises                 r steps up by 1 per chunk: the running maximum is replaced in every chunk
      one_key_tail              the last key carries the maximum; with Nkv = n * chunk + 1 it is the only valid key of the last chunk"""
    Cc = heads * hd
    q = torch.randn(B, Nq, Cc, generator=gen)
    kv = torch.randn(B, Nkv, 2 * Cc, generator=gen)
    j = torch.arange(Nkv, dtype=torch.float32)
    # the other ramps are <= 0 with the maximum at 0, so the winning scores stay small and their fp32 rounding error with them (softmax is shift-invariant)
    if kind == "max_last":
        r = 4.0 * (j + 1) / Nkv
        kv[..., :Cc] *= (0.02 + 0.1 * (j + 1) / Nkv)[None, :, None]
    elif kind == "max_first_rest_underflow":
        r = torch.where(j < 5, torch.tensor(0.0), torch.where(j >= chunk, torch.tensor(-40.0), torch.tensor(-2.0)))
        kv[..., :Cc] *= 0.1
    elif kind == "max_rises":
        r = torch.floor(j / chunk) - float((Nkv - 1) // chunk)
        kv[..., :Cc] *= 0.1
    elif kind == "one_key_tail":
        # a small gap and small key noise: the last key wins every row by >= 8*3*0.5 / sqrt(hd) >= 1.5 without saturating the softmax (a one-hot row's dq
        # is a cancelled sum that bf16 storage of `out` cannot carry, whatever the kernel)
        r = torch.full((Nkv,), -0.5); r[-1] = 0.0
        kv[..., :Cc] *= 0.02
    else:
        raise ValueError(kind)
    qv, kk = q.view(B, Nq, heads, hd), kv[..., :Cc].view(B, Nkv, heads, hd)
    qv[..., 0] = qv[..., 0].abs() + 3.0
    kk[..., 0] = r[None, :, None]
    return q * 8.0, kv
