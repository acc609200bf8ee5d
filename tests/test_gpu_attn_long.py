"""GPU tests of attention over more than 256 keys (pn2_attn_long_fwd / pn2_attn_long_bwd, csrc/pn2_attn.hip: keys streamed in 128-key chunks with an
online softmax): the C ABI against float64 torch at head_dim 32 and 64, fp32 and bf16, on shapes at the edges of the chunking and on rows built to
break a streaming softmax (tests/attnlongref.py); refusals; both kernel families on one input (and bit for bit up to one chunk); determinism; the fp32 dQ accumulation;
Engine.attention's routing; and the PVTv2 models, Trainer capture / replay and VolumePredictor at 544^2 and 288 x 960."""
import ctypes as C
import os
import sys
from collections import OrderedDict

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
os.environ.setdefault("PN2_NO_PRETRAINED", "1")
import attnlongref as A  # noqa: E402
import emcad_b0ref as R  # noqa: E402
from test_gpu_pvt import relmax, rell2  # noqa: E402

dev = "cuda"
CHUNK = 128                                             # AL_CK of csrc/pn2_attn.hip, both kernel routes, forward and backward
P_ = lambda t: C.c_void_p(t.data_ptr())


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()
    yield
    pn2.set_compute_dtype("bf16")


# ------------------------------------------------------------------------------------------ the C ABI against float64
def _launch(long, dtn, hd, heads, q, kv, do, pad_q, pad_kv):
    """One forward + backward through the long (or the short) entry points on NaN-padded views; returns the six device buffers."""
    from pn2 import capi, F32, BF16
    dt, tdt = (F32, torch.float32) if dtn == "fp32" else (BF16, torch.bfloat16)
    B, Nq, Cc = q.shape
    Nkv = kv.shape[1]
    ldq, ldkv = Cc + pad_q, 2 * Cc + pad_kv

    def view(t, rows, ld):                              # channel slice of a wider buffer; the columns past the slice hold NaN
        buf = torch.full((B, rows, ld), float("nan"), dtype=tdt, device=dev)
        if t is not None:
            buf[..., :t.shape[2]] = t.to(tdt)
        return buf
    qb, kvb, dob = view(q, Nq, ldq), view(kv, Nkv, ldkv), view(do, Nq, ldq)
    ob, dqb, dkvb = view(None, Nq, ldq), view(None, Nq, ldq), view(None, Nkv, ldkv)
    lse = torch.empty(B, heads, Nq, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sc = hd ** -0.5
    if long:
        n = (C.c_longlong * 3)()
        capi.call.pn2_attn_long_bwd_workspace(dt, B, Nq, heads, hd, n)
        assert n[0] == B * heads * capi.call.pn2_attn_long_bwd_blocks(dt, B, heads, Nq) * 2 * CHUNK * hd and n[1] == B * heads * Nq and n[2] == B * Nq * Cc
        part, delta, dqacc = (torch.empty(int(v), device=dev) for v in n)            # the layouts of pn2.h
        capi.call.pn2_attn_long_fwd(dt, P_(qb), ldq, P_(kvb), ldkv, P_(ob), ldq, P_(lse), B, Nq, Nkv, heads, hd, sc, st)
        capi.call.pn2_attn_long_bwd(dt, P_(qb), ldq, P_(kvb), ldkv, P_(ob), ldq, P_(dob), ldq, P_(lse), P_(dqb), ldq, P_(dkvb), ldkv, P_(part), P_(delta),
                                    P_(dqacc), B, Nq, Nkv, heads, hd, sc, st)
    else:
        nb = capi.call.pn2_attn_bwd_blocks(dt, B, heads, Nq)
        part = torch.empty(B, heads, nb, 2, (Nkv + 63) // 64 * 64, hd, device=dev)
        delta = torch.empty(B, heads, Nq, device=dev)
        capi.call.pn2_attn_fwd(dt, P_(qb), ldq, P_(kvb), ldkv, P_(ob), ldq, P_(lse), B, Nq, Nkv, heads, hd, sc, st)
        capi.call.pn2_attn_bwd(dt, P_(qb), ldq, P_(kvb), ldkv, P_(ob), ldq, P_(dob), ldq, P_(lse), P_(dqb), ldq, P_(dkvb), ldkv, P_(part), P_(delta),
                               B, Nq, Nkv, heads, hd, sc, st)
    torch.cuda.synchronize()
    return ob, dqb, dkvb, lse


_REF = {}


def _reference(dtn, hd, heads, q, kv, do, key):
    """float64 plain softmax on the (bf16-rounded) inputs: (out, dq, dkv, lse); computed once per input and shared."""
    if key in _REF:
        return _REF[key]
    B, Nq, Cc = q.shape
    Nkv = kv.shape[1]
    cast = (lambda t: t.bfloat16().double()) if dtn == "bf16" else (lambda t: t.double())
    q64, kv64 = cast(q).requires_grad_(True), cast(kv).requires_grad_(True)
    qq = q64.reshape(B, Nq, heads, hd).transpose(1, 2)
    kk = kv64.reshape(B, Nkv, 2, heads, hd).permute(2, 0, 3, 1, 4)
    s = (qq @ kk[0].transpose(-2, -1)) * hd ** -0.5
    r = (s.softmax(-1) @ kk[1]).transpose(1, 2).reshape(B, Nq, Cc)
    r.backward(cast(do))
    _REF[key] = (r.detach(), q64.grad, kv64.grad, torch.logsumexp(s.detach(), -1))
    return _REF[key]


def _data(heads, hd, Nq, Nkv, B=2, seed=None, kind=None):
    g = torch.Generator().manual_seed(heads * 1000 + Nq + Nkv if seed is None else seed)
    Cc = heads * hd
    if kind is None:
        q, kv = torch.randn(B, Nq, Cc, generator=g), torch.randn(B, Nkv, 2 * Cc, generator=g)
    else:
        q, kv = A.adversarial(kind, B, heads, Nq, Nkv, hd, CHUNK, g)
    return q, kv, torch.randn(B, Nq, Cc, generator=g)


def _errors(long, dtn, hd, heads, Nq, Nkv, pad_q, pad_kv, seed=None, kind=None):
    q, kv, do = _data(heads, hd, Nq, Nkv, seed=seed, kind=kind)
    Cc = heads * hd
    ob, dqb, dkvb, lse = _launch(long, dtn, hd, heads, q, kv, do, pad_q, pad_kv)
    r, gq, gkv, lref = _reference(dtn, hd, heads, q, kv, do, (dtn, hd, heads, Nq, Nkv, seed, kind))
    for t, n in ((ob, Cc), (dqb, Cc), (dkvb, 2 * Cc)):
        assert bool(torch.isnan(t[..., n:].float()).all()), "wrote past the row"
    err = relmax if dtn == "fp32" else rell2
    e = dict(out=err(ob[..., :Cc].float(), r), dq=err(dqb[..., :Cc].float(), gq), dkv=err(dkvb[..., :2 * Cc].float(), gkv),
             lse=float((lse.double().cpu() - lref).abs().max()))
    print(f"\n{'long' if long else 'short'} {dtn} hd{hd} h{heads} Nq{Nq} Nkv{Nkv} pad({pad_q},{pad_kv}) {kind or ''}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    return e


def _check(long, dtn, hd, heads, Nq, Nkv, pad_q, pad_kv, **kw):
    e = _errors(long, dtn, hd, heads, Nq, Nkv, pad_q, pad_kv, **kw)
    tol = 5e-5 if dtn == "fp32" else 3e-2                # the bounds of the project's attention tests (test_gpu_pvt.py, test_gpu_pvt_b0.py)
    assert e["out"] < tol, "forward"
    assert e["dq"] < tol, "dq"
    assert e["dkv"] < tol, "dkv"
    assert e["lse"] < (1e-4 if dtn == "fp32" else 5e-2)  # lse = row maximum + log of the sum, the meaning it has in pn2_attn_fwd (bf16: scores from rounded products)
    return e


def _all_views(long, dtn, hd, heads, Nq, Nkv, **kw):
    _check(long, dtn, hd, heads, Nq, Nkv, 0, 0, **kw)            # ld = heads * hd (the MFMA kernels for bf16)
    _check(long, dtn, hd, heads, Nq, Nkv, 16, 8, **kw)           # channel slice of a wider buffer
    if dtn == "bf16":
        _check(long, dtn, hd, heads, Nq, Nkv, 4, 12, **kw)       # ld not a multiple of 8: the scalar kernels


# (heads, Nq, Nkv): the first key past the short family, partial query tiles, whole and partial chunks, the top of the range; then chunk - 1, chunk, chunk + 1
LONG_CASES = [(1, 1, 257), (2, 63, 289), (5, 130, 384), (1, 130, 385), (2, 300, 512), (8, 63, 513), (1, 200, 1041), (2, 1, 4096),
              (2, 70, CHUNK - 1), (2, 70, CHUNK), (2, 70, CHUNK + 1)]


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("case", LONG_CASES)
def test_attention_long_c_abi(case, hd, dtn):
    _all_views(True, dtn, hd, *case)


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("kind", A.ADVERSARIAL)
def test_attention_long_rows_built_to_break_a_streaming_softmax(kind, hd, dtn):
    """q scaled by 8 (tests/attnlongref.py).  Nkv = 600 for every item; "exactly one valid key in the last chunk" cannot hold at 600 keys with 128-key
    chunks (600 = 4 * 128 + 88), so that item runs at 600 (the last key carries the maximum) AND at 4 * 128 + 1 = 513, where it is alone in its chunk."""
    _all_views(True, dtn, hd, 2, 130, 600, kind=kind)
    if kind == "one_key_tail":
        _all_views(True, dtn, hd, 2, 130, 4 * CHUNK + 1, kind=kind)


def test_attention_long_refusals():
    from pn2 import capi, BF16, F32
    lib = capi.load()
    buf = torch.zeros(1 << 20, device=dev)
    p, st = P_(buf), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = (C.c_longlong * 3)()
    for dt in (F32, BF16):
        for hd in (16, 48, 128):
            assert lib.pn2_attn_long_fwd(dt, p, 2 * hd, p, 4 * hd, p, 2 * hd, p, 1, 16, 300, 2, hd, 0.1, st) == -2, hd
            assert lib.pn2_attn_long_bwd(dt, p, 2 * hd, p, 4 * hd, p, 2 * hd, p, 2 * hd, p, p, 2 * hd, p, 4 * hd, p, p, p, 1, 16, 300, 2, hd, 0.1, st) == -2, hd
            assert lib.pn2_attn_long_bwd_workspace(dt, 1, 16, 2, hd, n) == -2
        for nkv in (0, 4097):
            assert lib.pn2_attn_long_fwd(dt, p, 64, p, 128, p, 64, p, 1, 16, nkv, 2, 32, 0.1, st) == -2, nkv
            assert lib.pn2_attn_long_bwd(dt, p, 64, p, 128, p, 64, p, 64, p, p, 64, p, 128, p, p, p, 1, 16, nkv, 2, 32, 0.1, st) == -2, nkv
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0, "a refused call wrote"


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("Nkv", [200, 256])
def test_both_families_meet_the_float64_bounds_on_one_input(Nkv, hd, dtn):
    for long in (False, True):
        _all_views(long, dtn, hd, 2, 130, Nkv)


@pytest.mark.parametrize("pads", [(0, 0), (16, 8)])
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("case", [(2, 130, 128), (1, 63, 100), (5, 70, 49)])
def test_both_families_give_the_same_bits_up_to_one_chunk(case, hd, pads):
    """bf16 MFMA route, at most 128 keys: one key range, a first-chunk factor of 0, the same slot count and slot order - the two families run the same
    arithmetic on every row, so out, lse, dq and dkv agree bit for bit."""
    heads, Nq, Nkv = case
    q, kv, do = _data(heads, hd, Nq, Nkv)
    short = _launch(False, "bf16", hd, heads, q, kv, do, *pads)
    long = _launch(True, "bf16", hd, heads, q, kv, do, *pads)
    Cc = heads * hd
    for name, x, y, n in zip(("out", "dq", "dkv", "lse"), short, long, (Cc, Cc, 2 * Cc, Nq)):
        x, y = x[..., :n].float(), y[..., :n].float()
        print(f"\n{name} hd{hd} {case} pad{pads}: max |short - long| {float((x - y).abs().max()):.3e}, {int((x != y).sum())} of {x.numel()} differ")
    for name, x, y, n in zip(("out", "dq", "dkv", "lse"), short, long, (Cc, Cc, 2 * Cc, Nq)):
        assert torch.equal(x[..., :n], y[..., :n]), name


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
@pytest.mark.parametrize("hd", [32, 64])
def test_attention_long_is_deterministic(hd, dtn):
    q, kv, do = _data(5, hd, 300, 1041)
    for pads in ((0, 0),) + (((4, 12),) if dtn == "bf16" else ()):
        a = _launch(True, dtn, hd, 5, q, kv, do, *pads)
        b = _launch(True, dtn, hd, 5, q, kv, do, *pads)
        Cc = 5 * hd
        for x, y, n in zip(a, b, (Cc, Cc, 2 * Cc, 300)):
            assert torch.equal(x[..., :n], y[..., :n])


@pytest.mark.parametrize("hd", [32, 64])
def test_dq_accumulates_in_fp32_across_key_ranges(hd):
    """bf16, (1, 130, 1041): nine key ranges.  The rel-L2 of dq against float64 may not exceed 1.5 x the figure of the existing kernels at (1, 130, 256)
    on the same seed - what one bf16 read-modify-write of dq per key range would fail."""
    seed = 4242
    long = _errors(True, "bf16", hd, 1, 130, 1041, 0, 0, seed=seed)["dq"]
    short = _errors(False, "bf16", hd, 1, 130, 256, 0, 0, seed=seed)["dq"]
    print(f"\ndq rel-L2 hd{hd}: long kernels at 1041 keys {long:.3e}, existing kernels at 256 keys {short:.3e}")
    assert long <= 1.5 * short


# ------------------------------------------------------------------------------------------ Engine.attention
def _engine_attention(dt, hd, heads, qhw, khw, seed):
    from pn2.engine import Engine
    from pn2.graph import _seed_grad
    torch.manual_seed(seed)
    B, Cc = 2, heads * hd
    q = torch.randn(B, Cc, *qhw, device=dev); kv = torch.randn(B, 2 * Cc, *khw, device=dev)
    eng = Engine(dt, True, need_grad=True)
    qa, kva = eng.from_nchw(q, True), eng.from_nchw(kv, True)
    o = eng.attention(qa, kva, heads)
    out = eng.to_nchw(o).clone()
    go = torch.randn_like(out)
    _seed_grad(o, go); eng.backward()
    return q, kv, go, qa, kva, o, out


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
@pytest.mark.parametrize("hd", [32, 64])
def test_attention_long_engine(hd, dtn):
    """Engine.attention above 256 keys: the maps of a 544^2 image's stage 1 / a 288 x 960 image's stage 3 / a 544^2 image's stage 4 (sr 2 / 2 / 1)."""
    from pn2 import F32, BF16
    dt = F32 if dtn == "fp32" else BF16
    err, tol = (relmax, 5e-5) if dt == F32 else (rell2, 3e-2)
    for (qh, qw), (kh, kw) in (((34, 34), (17, 17)), ((18, 60), (9, 30)), ((17, 17), (17, 17))):
        for heads in (1, 5):
            q, kv, go, qa, kva, _, out = _engine_attention(dt, hd, heads, (qh, qw), (kh, kw), heads)
            B, Cc, Nq, Nkv = 2, heads * hd, qh * qw, kh * kw
            cast = (lambda t: t.bfloat16().float()) if dt == BF16 else (lambda t: t)
            q64 = cast(q).double().cpu().requires_grad_(True); kv64 = cast(kv).double().cpu().requires_grad_(True)
            qq = q64.flatten(2).transpose(1, 2).reshape(B, Nq, heads, hd).permute(0, 2, 1, 3)
            kk = kv64.flatten(2).transpose(1, 2).reshape(B, Nkv, 2, heads, hd).permute(2, 0, 3, 1, 4)
            r = (((qq @ kk[0].transpose(-2, -1)) * hd ** -0.5).softmax(dim=-1) @ kk[1]).transpose(1, 2).reshape(B, Nq, Cc).transpose(1, 2).reshape(B, Cc, qh, qw)
            r.backward(go.double().cpu())
            assert err(out, r) < tol
            assert err(qa.grad.float().permute(0, 3, 1, 2), q64.grad) < tol
            assert err(kva.grad.float().permute(0, 3, 1, 2), kv64.grad) < tol


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
def test_engine_routes_256_keys_to_the_short_entry_points(dtn):
    """16 x 16 keys: Engine.attention's output and gradients are those of a direct pn2_attn_fwd / pn2_attn_bwd call, bit for bit."""
    from pn2 import capi, F32, BF16
    dt = F32 if dtn == "fp32" else BF16
    hd, heads, B = 32, 2, 2
    Cc = heads * hd
    q, kv, go, qa, kva, o, _ = _engine_attention(dt, hd, heads, (20, 20), (16, 16), 11)
    Nq, Nkv = 400, 256
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tdt = torch.float32 if dt == F32 else torch.bfloat16
    ob, dqb, dkvb = torch.empty(B, Nq, Cc, dtype=tdt, device=dev), torch.empty(B, Nq, Cc, dtype=tdt, device=dev), torch.empty(B, Nkv, 2 * Cc, dtype=tdt, device=dev)
    lse = torch.empty(B, heads, Nq, device=dev); delta = torch.empty(B, heads, Nq, device=dev)
    part = torch.empty(B, heads, capi.call.pn2_attn_bwd_blocks(dt, B, heads, Nq), 2, 256, hd, device=dev)
    do = go.permute(0, 2, 3, 1).reshape(B, Nq, Cc).to(tdt).contiguous()
    capi.call.pn2_attn_fwd(dt, qa.ptr, Cc, kva.ptr, 2 * Cc, P_(ob), Cc, P_(lse), B, Nq, Nkv, heads, hd, hd ** -0.5, st)
    capi.call.pn2_attn_bwd(dt, qa.ptr, Cc, kva.ptr, 2 * Cc, P_(ob), Cc, P_(do), Cc, P_(lse), P_(dqb), Cc, P_(dkvb), 2 * Cc, P_(part), P_(delta),
                           B, Nq, Nkv, heads, hd, hd ** -0.5, st)
    torch.cuda.synchronize()
    assert torch.equal(o.t.reshape(B, Nq, Cc), ob)
    assert torch.equal(qa.grad.reshape(B, Nq, Cc), dqb) and torch.equal(kva.grad.reshape(B, Nkv, 2 * Cc), dkvb)


# ------------------------------------------------------------------------------------------ models
def _b0(mode, train=True):
    import pn2
    from lib.networks import EMCADNet
    pn2.set_compute_dtype(mode)
    m = EMCADNet(num_classes=9, kernel_sizes=[1, 3, 5], expansion_factor=2, dw_parallel=True, add=True, lgag_ks=3, activation="relu6", encoder="pvt_v2_b0",
                 pretrain=False, dual=True)
    m.load_state_dict(R.state_dict(seed=5), strict=True)
    m.backbone.reset_drop_path(0.0)
    return m.to(dev).train(train)


_ORACLE = {}
# parameter-gradient probes next to the input gradient: attention weights of the first and the last stage
PROBES = ("backbone.block1.0.attn.q.weight", "backbone.block1.0.attn.kv.weight", "backbone.block4.1.attn.kv.weight")


def _b0_oracle(H, W):
    """oracle/emcad_oracle.py in float64 and float32 on the CPU for a 1 x 3 x H x W image (three channels: no 1 -> 3 stem, networks.py): the maps, the
    input gradient and the probe gradients of sum(maps * g), once per size."""
    if (H, W) not in _ORACLE:
        from oracle import emcad_oracle as E
        from oracle.pranet_oracle import Ctx, pvt_features
        g = torch.Generator().manual_seed(H + W)
        x = torch.randn(1, 3, H, W, generator=g)
        gys = [torch.randn(1, 9, H, W, generator=g) * 1e-3 for _ in range(8)]
        res = {}
        for dtp in (torch.float64, torch.float32):
            P = {k: (v.to(dtp) if v.is_floating_point() else v.clone()) for k, v in R.state_dict(seed=5).items()}
            for k in PROBES:
                P[k].requires_grad_(True)
            xx = x.detach().clone().to(dtp).requires_grad_(True)          # a leaf of its own: x itself must stay free of autograd state
            x1, x2, x3, x4 = pvt_features(P, "backbone.", xx, R.PVT_B0)
            lows = E.emcad_dual(P, "decoder.", x4, [x3, x2, x1], Ctx(True))
            outs = [torch.nn.functional.interpolate(o, scale_factor=s, mode="bilinear") for o, s in zip(lows, [32, 16, 8, 4] * 2)]
            sum((o * gy.to(dtp)).sum() for o, gy in zip(outs, gys)).backward()
            grads = {k: P[k].grad.double() for k in PROBES}
            grads["input"] = xx.grad.double()
            res[dtp] = ([o.detach() for o in outs], grads)
        _ORACLE[(H, W)] = (x, gys, res)
    return _ORACLE[(H, W)]


def _b0_run(mode, x, gys):
    model = _b0(mode)
    xg = x.detach().clone().to(dev).requires_grad_(True)
    outs = model(xg, mode="train")
    sum((o * gy.to(dev)).sum() for o, gy in zip(outs, gys)).backward()
    names = dict(model.named_parameters())
    grads = {k: names[k].grad.detach().double().cpu() for k in PROBES}
    assert xg.grad is not None, "the module surface returned no input gradient"
    grads["input"] = xg.grad.detach().double().cpu()
    return [o.detach() for o in outs], grads


@pytest.mark.parametrize("HW", [(544, 544), (288, 960)], ids=["544x544", "288x960"])
def test_emcadnet_b0_above_512_vs_oracle(HW):
    """EMCADNet(pvt_v2_b0, dual, K = 9), train mode, 1 x 3 x 544 x 544 (289 keys in every stage) and 1 x 3 x 288 x 960 (270 keys), against the oracle in
    float64 under the rules of test_gpu_pvt_b0.py.  fp32: maps within max(1e-4, 3 x the fp32 oracle's own distance to float64); the input gradient and the
    gradient probes within max(1e-4 relative, 3 x that distance) + 2e-6.  bf16: that file's band (rel-L2 < 0.35 per map) against the float64 maps and
    against this project's fp32 maps, finite gradients."""
    x, gys, res = _b0_oracle(*HW)
    o64, g64 = res[torch.float64]
    o32, g32 = res[torch.float32]
    outs, gp = _b0_run("fp32", x, gys)
    for i, o in enumerate(outs):
        own = float((o32[i].double() - o64[i]).abs().max())
        err = float((o.double().cpu() - o64[i]).abs().max())
        print(f"\nmap {i}: |ours - f64| {err:.2e}, the fp32 oracle's own {own:.2e}")
        assert tuple(o.shape) == tuple(o64[i].shape)
        assert err <= max(1e-4, 3 * own), i
    for k in ("input",) + PROBES:
        err, own, nrm = float((gp[k] - g64[k]).norm()), float((g32[k] - g64[k]).norm()), float(g64[k].norm())
        print(f"\ngradient {k}: |ours - f64| {err:.2e}, the fp32 oracle's own {own:.2e}, |f64| {nrm:.2e}")
        assert tuple(gp[k].shape) == tuple(g64[k].shape)
        assert err <= max(1e-4 * nrm, 3 * own) + 2e-6, k
    outs16, gp16 = _b0_run("bf16", x, gys)
    for i, o in enumerate(outs16):
        assert rell2(o, o64[i]) < 0.35 and rell2(o, outs[i]) < 0.35, i
    assert all(bool(torch.isfinite(v).all()) for v in gp16.values())


def test_pvt_pranet_v2_b2_544_vs_oracle_fp32():
    """PVT_PraNet_V2 (b2, head_dim 64) at 1 x 3 x 544 x 544, fp32, against oracle/pranet_oracle.py under the fp32 rule of test_gpu_pvt.py."""
    import pn2
    from lib.pranet import PVT_PraNet_V2
    from oracle import weights as W
    from oracle import pranet_oracle as O
    pn2.set_compute_dtype("fp32")
    sd = W.make_state_dict(W.manifest_pvt_pranet_v2(1), seed=3)
    model = PVT_PraNet_V2(num_class=1)
    model.load_state_dict(sd, strict=True)
    model.backbone.reset_drop_path(0.0)
    model = model.to(dev).train()
    x, _ = W.synthetic_batch(1, 544, seed=4321)
    with torch.no_grad():
        outs = model(x.to(dev))
        ref = {dtp: O.pvt_pranet_v2_forward({k: (v.to(dtp) if v.is_floating_point() else v.clone()) for k, v in sd.items()}, x.to(dtp), True)
               for dtp in (torch.float64, torch.float32)}
    for i, o in enumerate(outs):
        r64 = ref[torch.float64][i]
        own = float((ref[torch.float32][i].double() - r64).abs().max())
        err = float((o.double().cpu() - r64).abs().max())
        print(f"\nmap {i}: |ours - f64| {err:.2e}, the fp32 oracle's own {own:.2e}")
        assert err <= max(1e-4, 3 * own), i


def test_trainer_b0_544_capture_replays_bit_identically():
    """Trainer on the b0 model at 2 x 544^2, bf16: capture, three replays; loss and every gradient identical across replays and equal to the eager step."""
    from pn2.trainer import Trainer
    g = torch.Generator().manual_seed(77)
    N, S, K = 2, 544, 9
    x = torch.randn(N, 1, S, S, generator=g).to(dev)
    lab = torch.randint(0, K, (N, S // 16, S // 16), generator=g).to(dev)
    lab = torch.nn.functional.interpolate(lab[:, None].float(), size=(S, S), mode="nearest")[:, 0].long()
    bg = torch.stack([(lab != k).float() for k in range(K)], 1)

    def trainer():
        m = _b0("bf16")
        return Trainer(m, lr=0.0, clip=None, weight_decay=0.0, loss="mutation", hot=m.hot_parameters(True))
    eager = trainer()
    le = eager.forward_backward(x, (lab, bg)).clone(); ge = eager.gflat.clone()
    assert torch.isfinite(le).all() and torch.isfinite(ge).all() and float(ge.abs().max()) > 0
    cap = trainer()
    cap.capture(x, (lab, bg), warmup=2)
    for i in range(3):
        lg = cap.replay(x, (lab, bg))
        torch.cuda.synchronize()
        assert torch.equal(lg, le), i
        assert torch.equal(cap.gflat, ge), i


def test_volume_predictor_544():
    """VolumePredictor on a 3 x 544 x 544 volume, patch 544^2, batch 2 (the second batch filled with a zero slice): labels byte for byte those of
    voleval._predict_volume on the same batches."""
    import pn2
    import volevalref as VR
    from lib.networks import EMCADNet
    from oracle import weights as W
    from pn2 import voleval as V
    from pn2.infer import VolumePredictor
    pn2.set_compute_dtype("bf16")
    m = EMCADNet(num_classes=9, kernel_sizes=[1, 3, 5], expansion_factor=2, dw_parallel=True, add=True, lgag_ks=3, activation="relu6", encoder="pvt_v2_b0",
                 pretrain=False, dual=True)
    manifest = OrderedDict((k, tuple(v.shape)) for k, v in m.state_dict().items())
    m.load_state_dict(VR.nontrivial_bn_stats(W.make_state_dict(manifest, seed=5), seed=17), strict=True)
    m.backbone.reset_drop_path(0.0)
    m = m.to(dev).eval()
    patch, batch = (544, 544), 2
    image = torch.randn(3, 544, 544, generator=torch.Generator().manual_seed(31)).to(dev)
    full = torch.cat([image, image.new_zeros(1, 544, 544)])
    want = V._predict_volume(full, m, patch, lambda outs, single: V.predict_labels(list(outs)[:4], "sum_fg"), batch)[:3]
    got = VolumePredictor(m, patch_size=patch, batch_size=batch).predict(image, "sum_fg")
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 544, 544)
    assert torch.equal(got, want)
