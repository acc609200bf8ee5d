"""GPU parity tests (run with -m gpu on an MI355X): every HIP op, the model blocks, the whole PraNet-V2 training step and
the eval tail are compared — through the C ABI — with the CPU oracle on the same seeded inputs and with the committed golden
vectors that the imported reference produced.

Tolerances
  fp32 path (fp32 storage, conv contractions accumulated in double on v_mfma_f64_16x16x4_f64): single ops / blocks 5e-5 relative.
  Whole network in train mode: batch-statistics BN over a 2-image batch makes the fp32 problem ill-conditioned — the reference's own
  fp32 CPU result differs from the same reference run in float64 by up to 1.6e-3 on the logits (measured in tests/golden/make_golden.py,
  stored as f64.*), so "1e-4 abs against the reference's fp32 logits" (north star) cannot be met by ANY fp32 implementation, the
  reference re-run with another BLAS included.  What is gated instead, against the float64 run of the reference:
      |ours - ref64| <= max(1e-4, 0.6 * |ref32 - ref64|)      logits and losses  (measured: 0.25-0.4 x the reference's own gap)
      rel-L2(ours, ref64) <= max(2e-6, 1.0 * rel-L2(ref32, ref64))   every gradient probe, no outliers; median <= 0.8 x  (measured 0.23-0.63 x)
  i.e. this implementation must be CLOSER to the exact result than the reference's own fp32 path is.
  bf16 path: relative L2 <= 3e-2 per op (max-norm is meaningless once a ReLU mask bit flips on a near-zero activation); whole model:
  see test_model_bf16_vs_reference_f64.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
os.environ.setdefault("PN2_NO_PRETRAINED", "1")
dev = "cuda"


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()      # fails loudly if the HIP extension is missing
    yield
    pn2.set_compute_dtype("bf16")


def relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def rell2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


CONVS = [  # N, Cin, Cout, k, stride, pad, dil, H, W, bn, relu
    (2, 3, 32, 3, 2, 1, 1, 38, 38, False, False), (2, 32, 64, 3, 1, 1, 1, 19, 21, False, False), (2, 64, 256, 1, 1, 0, 1, 17, 17, False, False),
    (2, 256, 104, 1, 1, 0, 1, 9, 9, True, True), (3, 56, 56, 3, 2, 1, 1, 15, 15, True, True), (2, 256, 256, 5, 1, 2, 1, 11, 11, True, False),
    (2, 32, 32, (1, 5), 1, (0, 2), 1, 11, 11, True, False), (2, 32, 32, (7, 1), 1, (3, 0), 1, 11, 11, True, False),
    (2, 32, 32, 3, 1, 5, 5, 22, 22, True, False), (2, 128, 32, 3, 1, 1, 1, 22, 22, True, True), (1, 2048, 832, 1, 1, 0, 1, 11, 11, False, False),
    (1, 8, 8, 3, 1, 1, 1, 1, 1, False, False),      # single pixel
]


@pytest.mark.parametrize("dtn", ["fp32", "fp32fast", "bf16"])
@pytest.mark.parametrize("cfg", CONVS)
def test_conv_bn_act_fwd_bwd(dtn, cfg):
    from pn2 import F32, BF16
    from pn2.capi import F32F
    from pn2.engine import Engine
    from pn2.graph import _seed_grad
    N, Cin, Cout, k, stride, pad, dil, H, Wd, bn, relu = cfg
    dt = {"fp32": F32, "fp32fast": F32F, "bf16": BF16}[dtn]
    err, tol = (relmax, 3e-5) if dt != BF16 else (rell2, 5e-2)
    torch.manual_seed(1)
    conv = nn.Conv2d(Cin, Cout, k, stride, pad, dil, bias=False).to(dev)
    bnm = nn.BatchNorm2d(Cout).to(dev) if bn else None
    if bn:
        bnm.weight.data.uniform_(0.5, 1.5); bnm.bias.data.normal_(0, 0.2)
    x = torch.randn(N, Cin, H, Wd, device=dev)
    eng = Engine(dt, True, need_grad=True)
    a = eng.from_nchw(x, requires_grad=True)
    y = eng.conv_bn_act(a, conv, bnm, relu=relu)
    out = eng.to_nchw(y).clone()
    gy = torch.randn_like(out)
    _seed_grad(y, gy)
    eng.backward()
    gx = a.grad[..., :Cin].float().permute(0, 3, 1, 2)
    xc = x.double().cpu().requires_grad_(True)
    wc = conv.weight.detach().double().cpu().requires_grad_(True)
    r = F.conv2d(xc, wc, None, stride, pad, dil)
    if bn:
        g_ = bnm.weight.detach().double().cpu().requires_grad_(True); b_ = bnm.bias.detach().double().cpu().requires_grad_(True)
        r = F.batch_norm(r, None, None, g_, b_, True, 0.1, 1e-5)
    if relu:
        r = F.relu(r)
    r.backward(gy.double().cpu())
    assert err(out, r) < tol
    assert err(gx, xc.grad) < tol
    assert err(eng.pgrads.get(conv.weight), wc.grad) < tol
    if bn:
        assert err(eng.pgrads.get(bnm.weight), g_.grad) < tol
        assert err(eng.pgrads.get(bnm.bias), b_.grad) < tol


EVAL_CONVS = [  # N, Cin, Cout, k, stride, pad, H, W, relu, residual, out_map
    (2, 64, 256, 1, 1, 0, 17, 17, True, True, None), (3, 104, 26, 3, 1, 1, 15, 13, True, False, (26, 32)), (2, 32, 64, 3, 2, 1, 19, 21, 2, False, None),
    (1, 256, 256, 5, 1, 2, 11, 11, False, False, None), (2, 40, 48, 3, 1, 1, 9, 9, 2, True, None), (1, 2048, 832, 1, 1, 0, 11, 11, True, False, None),
]


@pytest.mark.parametrize("dtn", ["fp32", "fp32fast", "bf16"])
@pytest.mark.parametrize("cfg", EVAL_CONVS)
def test_eval_conv_bn_fused_in_gemm_epilogue(dtn, cfg, monkeypatch):
    """Eval-mode conv + BatchNorm (+ ReLU / ReLU6) (+ residual) in ONE launch (pn2_conv_gemm_affine, MyTest_med.py:98-104) against the two-launch path
    (conv -> raw, pn2_affine_act) and against torch float64: fp32 bit-identical to the two launches; bf16 at least as close to float64
    (one rounding fewer; with a residual: the same two roundings at other places, within 1.25 x).  Covers group-padded outputs (26 channels in 32 slots), partial last tiles, stride 2, a 5x5 and the split between pre- and post-residual
    activation."""
    from pn2 import F32, BF16
    from pn2.capi import F32F
    from pn2 import engine as E, core
    N, Cin, Cout, k, stride, pad, H, Wd, relu, use_res, omap = cfg
    dt = {"fp32": F32, "fp32fast": F32F, "bf16": BF16}[dtn]
    torch.manual_seed(2)
    conv = nn.Conv2d(Cin, Cout, k, stride, pad, bias=False).to(dev)
    bnm = nn.BatchNorm2d(Cout).to(dev).eval()
    bnm.weight.data.uniform_(0.5, 1.5); bnm.bias.data.normal_(0, 0.3); bnm.running_mean.normal_(0, 0.5); bnm.running_var.uniform_(0.5, 2.0)
    x = torch.randn(N, Cin, H, Wd, device=dev)
    OH, OW = (H + 2 * pad - k) // stride + 1, (Wd + 2 * pad - k) // stride + 1
    res = torch.randn(N, Cout, OH, OW, device=dev) if use_res else None

    def run(fuse):
        monkeypatch.setattr(core, "EVAL_FUSE", fuse)
        eng = E.Engine(dt, False, need_grad=False)
        a = eng.from_nchw(x)
        r = eng.from_nchw(res) if use_res else None
        y = eng.conv_bn_act(a, conv, bnm, relu=relu, residual=r, out_map=omap)
        torch.cuda.synchronize()
        return eng.to_nchw(y).clone(), y.t.clone()
    (y1, t1), (y0, t0) = run(True), run(False)
    xr = x if dt != BF16 else x.bfloat16().float()
    wr = conv.weight.detach() if dt != BF16 else conv.weight.detach().bfloat16().float()
    ref = F.batch_norm(F.conv2d(xr.double().cpu(), wr.double().cpu(), None, stride, pad), bnm.running_mean.double().cpu(), bnm.running_var.double().cpu(),
                       bnm.weight.detach().double().cpu(), bnm.bias.detach().double().cpu(), False, 0.1, 1e-5)
    if use_res:
        ref = ref + (res if dt != BF16 else res.bfloat16().float()).double().cpu()
    ref = F.relu6(ref) if relu == 2 else (F.relu(ref) if relu else ref)
    if dt != BF16:
        assert torch.equal(t1, t0)                     # same fma on the same correctly rounded conv result
        assert relmax(y1, ref) < 3e-5
    else:
        # (with a residual the fused form rounds BN(conv) to bf16 before the add - the two-launch form rounds the raw conv output instead: two roundings
        # either way, the same size of error; without one the fused form saves a rounding)
        assert rell2(y1, y0) < 6e-3 and rell2(y1, ref) <= rell2(y0, ref) * (1.25 if use_res else 1.02) + 1e-6, (rell2(y1, ref), rell2(y0, ref))
        if omap is not None:                           # pad slots of a group-padded output stay exact zeros
            assert float(t1[..., Cout:].abs().max()) == 0.0


@pytest.mark.parametrize("dtn", ["fp32", "fp32fast", "bf16"])
def test_reverse_attention_gate_in_gemm_epilogue(dtn):
    """V1 reverse attention (PraNet_Res2Net.py:153-155): ra_conv1((1 - sigmoid(crop)).expand(C) * x_l) with a 1x1 ra_conv1 + train-mode BN.  The fused
    path scales the GEMM's accumulator rows (pn2_conv_gemm_gated) and never writes the gated copy of x_l; outputs and all four gradients (x_l, crop,
    conv weight, BN affine) against torch float64 autograd, and against the engine's own materialising path (pn2_ra_gate_fwd / _bwd)."""
    from pn2 import F32, BF16
    from pn2.capi import F32F
    from pn2.engine import Engine, Act
    from pn2.graph import _seed_grad
    dt = {"fp32": F32, "fp32fast": F32F, "bf16": BF16}[dtn]
    err, tol = (relmax, 5e-5) if dt != BF16 else (rell2, 3e-2)
    torch.manual_seed(11)
    N, H, Wd, Cin, Cout = 3, 11, 13, 136, 64
    conv = nn.Conv2d(Cin, Cout, 1, bias=False).to(dev); bnm = nn.BatchNorm2d(Cout).to(dev)
    bnm.weight.data.uniform_(0.5, 1.5); bnm.bias.data.normal_(0, 0.3)
    x = torch.randn(N, Cin, H, Wd, device=dev)
    crop = 2.0 * torch.randn(N, 1, H, Wd, device=dev)
    gy = torch.randn(N, Cout, H, Wd, device=dev)

    def run(fused):
        eng = Engine(dt, True, need_grad=True)
        a = eng.from_nchw(x, requires_grad=True)
        c = Act(eng, crop.reshape(N, H, Wd, 1).clone(), 1, 1, 1, F32, requires_grad=True)
        y = eng.conv_bn_act(a, conv, bnm, gate=c) if fused else eng.conv_bn_act(eng.ra_gate(a, c), conv, bnm)
        out = eng.to_nchw(y).clone()
        _seed_grad(y, gy)
        eng.backward()
        return out, [a.grad[..., :Cin].float().permute(0, 3, 1, 2).clone(), c.grad.reshape(N, 1, H, Wd).clone()] + \
            [eng.pgrads.get(p_).clone() for p_ in (conv.weight, bnm.weight, bnm.bias)]

    rm0, rv0 = bnm.running_mean.clone(), bnm.running_var.clone()
    out, grads = run(True)
    cast = (lambda t: t.bfloat16().double()) if dt == BF16 else (lambda t: t.double())
    xc, cc = cast(x).cpu().requires_grad_(True), crop.double().cpu().requires_grad_(True)
    cr, br = nn.Conv2d(Cin, Cout, 1, bias=False).double(), nn.BatchNorm2d(Cout).double()
    cr.weight.data.copy_(cast(conv.weight.data).cpu()); br.weight.data.copy_(bnm.weight.data.double().cpu()); br.bias.data.copy_(bnm.bias.data.double().cpu())
    r = br(cr((1 - torch.sigmoid(cc)).expand(-1, Cin, -1, -1) * xc))
    r.backward(gy.double().cpu())
    ref = [xc.grad, cc.grad, cr.weight.grad, br.weight.grad, br.bias.grad]
    assert err(out, r) < tol
    for i_, (g_, r_) in enumerate(zip(grads, ref)):
        if float(r_.abs().max()) > 1e-9:
            assert err(g_, r_) < tol, (i_, err(g_, r_))
    assert relmax(bnm.running_var, br.running_var) < (1e-5 if dt != BF16 else 2e-2)
    bnm.running_mean.copy_(rm0); bnm.running_var.copy_(rv0)
    out0, grads0 = run(False)
    assert err(out, out0) < (1e-5 if dt != BF16 else 2e-2)
    for g_, g0 in zip(grads, grads0):
        if float(g0.abs().max()) > 1e-9:
            assert err(g_, g0) < (2e-5 if dt != BF16 else 3e-2)


@pytest.mark.parametrize("dtn", ["fp32", "fp32fast", "bf16"])
@pytest.mark.parametrize("case", ["chain", "residual", "big_mean"])
def test_bn_backward_statistics_in_dgrad_epilogue(dtn, case, monkeypatch):
    """conv -> BN -> ReLU -> conv -> BN [-> + residual -> ReLU -> conv]: with x_last=True the second (third) conv's dgrad GEMM takes the
    BatchNorm-backward sums of the layer below in its epilogue (pn2_conv_gemm_ep) instead of a pn2_bn_bwd_reduce pass; same gradients as
    torch float64 autograd, and - in fp32 - as the engine's own reduce-pass path.  big_mean: |mean| >> sigma channels (the Chan-merged
    forward statistics must not cancel)."""
    from pn2 import F32, BF16, engine, core
    from pn2.capi import F32F
    from pn2.engine import Engine
    from pn2.graph import _seed_grad
    from pn2 import capi
    dt = {"fp32": F32, "fp32fast": F32F, "bf16": BF16}[dtn]
    err, tol = (relmax, 5e-5) if dt != BF16 else (rell2, 1e-1)         # bf16: three BatchNorm layers deep
    torch.manual_seed(5)
    N, H, Wd, C0, C1, C2 = 3, 13, 17, 24, 40, 56
    c1 = nn.Conv2d(C0, C1, 3, 1, 1, bias=False).to(dev); b1 = nn.BatchNorm2d(C1).to(dev)
    c2 = nn.Conv2d(C1, C1 if case == "residual" else C2, 3 if case != "residual" else 1, 1, 1 if case != "residual" else 0, bias=False).to(dev)
    b2 = nn.BatchNorm2d(c2.out_channels).to(dev)
    c3 = nn.Conv2d(c2.out_channels, 32, 1, bias=False).to(dev); b3 = nn.BatchNorm2d(32).to(dev)
    for b in (b1, b2, b3):
        b.weight.data.uniform_(0.5, 1.5); b.bias.data.normal_(0, 0.3)
    x = torch.randn(N, C0, H, Wd, device=dev)
    if case == "big_mean":
        x = x + 6.0
        c1.weight.data.abs_()          # conv1's outputs: |mean| ~ 25 sigma in every channel

    def run(x_last):
        eng = Engine(dt, True, need_grad=True)
        a = eng.from_nchw(x, requires_grad=True)
        launched = []
        real = capi.call.pn2_conv_gemm_ep
        monkeypatch.setattr(capi.call, "pn2_conv_gemm_ep", lambda *aa: (launched.append(1), real(*aa))[1], raising=False)
        y1 = eng.conv_bn_act(a, c1, b1, relu=True)
        if case == "residual":
            y2 = eng.conv_bn_act(y1, c2, b2, relu=True, residual=y1, x_last=x_last)       # y1 feeds the conv first, then the residual add
            y3 = eng.conv_bn_act(y2, c3, b3, relu=False, x_last=x_last)
        else:
            y2 = eng.conv_bn_act(y1, c2, b2, relu=False, x_last=x_last)
            y3 = eng.conv_bn_act(y2, c3, b3, relu=True, x_last=x_last)
        out = eng.to_nchw(y3).clone()
        gy = torch.randn(out.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(9))
        _seed_grad(y3, gy)
        eng.backward()
        grads = [a.grad[..., :C0].float().permute(0, 3, 1, 2).clone()] + [eng.pgrads.get(p_).clone() for m_ in (c1, b1, c2, b2, c3, b3) for p_ in m_.parameters()]
        return out, gy, grads, len(launched)

    out, gy, grads, n_ep = run(True)
    assert n_ep == 2, "the epilogue path did not run"
    xc = x.double().cpu().requires_grad_(True)
    mods = [m_.double().cpu() for m_ in (nn.Conv2d(C0, C1, 3, 1, 1, bias=False), nn.BatchNorm2d(C1), nn.Conv2d(C1, c2.out_channels, c2.kernel_size, 1, c2.padding, bias=False),
                                        nn.BatchNorm2d(c2.out_channels), nn.Conv2d(c2.out_channels, 32, 1, bias=False), nn.BatchNorm2d(32))]
    for m_, src in zip(mods, (c1, b1, c2, b2, c3, b3)):
        m_.load_state_dict({k: v.double().cpu() for k, v in src.state_dict().items()}); m_.train()
    r1 = F.relu(mods[1](mods[0](xc)))
    if case == "residual":
        r2 = F.relu(mods[3](mods[2](r1)) + r1); r3 = mods[5](mods[4](r2))
    else:
        r2 = mods[3](mods[2](r1)); r3 = F.relu(mods[5](mods[4](r2)))
    r3.backward(gy.double().cpu())
    ref = [xc.grad] + [p_.grad for m_ in mods for p_ in m_.parameters()]
    if case == "big_mean":
        if dt == BF16:
            return                  # bf16 storage of a tensor with |mean| >> sigma has no meaningful reference; fp32 checks the statistics
        tol = 2e-3                  # the fp32 rounding of the conv outputs themselves is amplified by |mean| / sigma
    assert err(out, r3) < tol
    for i_, (g_, r_) in enumerate(zip(grads, ref)):
        if float(r_.abs().max()) > 1e-9:          # (the bias of a BatchNorm behind a 1x1 conv + train-mode BatchNorm has an exactly-zero gradient)
            assert err(g_, r_) < tol, (i_, err(g_, r_))
    # against the separate reduce pass: same sums up to fp32 summation order (bf16: the epilogue sees the fp32 gradient tile before it is rounded)
    monkeypatch.setattr(core, "BNB_EPILOGUE", False)
    out0, _, grads0, n0 = run(True)
    assert n0 == 0
    for g_, r_, f_ in zip(grads, grads0, ref):
        if float(f_.abs().max()) > 1e-9:
            if dt != BF16:
                assert relmax(g_, r_) < (2e-5 if case != "big_mean" else 2e-3)
            else:
                assert rell2(g_, r_) < 3e-2


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
def test_pool_and_bilinear_ops(dtn):
    from pn2 import F32, BF16
    from pn2.engine import Engine
    from pn2.graph import _seed_grad
    dt = F32 if dtn == "fp32" else BF16
    err, tol = (relmax, 1e-5) if dt == F32 else (rell2, 1e-2)
    torch.manual_seed(2)

    def run(build, ref, x):
        eng = Engine(dt, True, need_grad=True)
        a = eng.from_nchw(x, True)
        y = build(eng, a)
        o = eng.to_nchw(y).clone(); g = torch.randn_like(o); _seed_grad(y, g); eng.backward()
        xc = (x.bfloat16().float() if dt == BF16 else x).cpu().requires_grad_(True)
        r = ref(xc); r.backward(g.cpu())
        assert err(o, r) < tol
        assert err(a.grad.float().permute(0, 3, 1, 2), xc.grad) < tol
    run(lambda e, a: e.maxpool3x3s2(a), lambda t: F.max_pool2d(t, 3, 2, 1), torch.randn(2, 16, 13, 15, device=dev))
    for (k, s, p, ceil, inc, H) in ((3, 1, 1, False, True, 12), (3, 2, 1, False, True, 13), (2, 2, 0, True, False, 13), (2, 2, 0, True, False, 12)):
        run(lambda e, a: e.avgpool(a, k, s, p, ceil, inc), lambda t: F.avg_pool2d(t, k, s, p, ceil, inc), torch.randn(2, 8, H, H + 1, device=dev))
    for (scale, ac, C, H) in ((2, True, 32, 11), (2, False, 8, 11), (0.25, False, 8, 44), (8, False, 8, 11), (32, False, 8, 5), (16, False, 8, 3)):
        run(lambda e, a: e.bilinear(a, scale, ac), lambda t: F.interpolate(t, scale_factor=scale, mode="bilinear", align_corners=ac), torch.randn(2, C, H, H, device=dev))


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
def test_product_backward_one_pass_matches_two_launches_and_torch(dtn, monkeypatch):
    """eng.mul's backward (pn2_mul_bwd: both operand gradients from one pass over dy) = the two pn2_binary launches, bit for bit, fresh and accumulating."""
    from pn2 import F32, BF16, core
    from pn2.engine import Engine
    from pn2.graph import _seed_grad
    dt = F32 if dtn == "fp32" else BF16
    torch.manual_seed(5)
    xa, xb = torch.randn(2, 24, 9, 11, device=dev), torch.randn(2, 24, 9, 11, device=dev)
    g = torch.randn(2, 24, 9, 11, device=dev)

    def run(one_pass):
        monkeypatch.setattr(core, "MUL_BWD", one_pass)
        eng = Engine(dt, True, need_grad=True)
        a, b = eng.from_nchw(xa, True), eng.from_nchw(xb, True)
        y = eng.add(eng.mul(a, b), eng.mul(b, a))          # the second product accumulates into both gradients
        _seed_grad(y, g); eng.backward()
        return a.grad.clone(), b.grad.clone()
    (a1, b1), (a2, b2) = run(True), run(False)
    assert torch.equal(a1, a2) and torch.equal(b1, b2)
    q = (lambda t: t.bfloat16().float()) if dt == BF16 else (lambda t: t)
    tol = 1e-5 if dt == F32 else 2e-2
    assert relmax(a1.float().permute(0, 3, 1, 2), 2 * q(g) * q(xb)) < tol and relmax(b1.float().permute(0, 3, 1, 2), 2 * q(g) * q(xa)) < tol


def test_dsra_fusion_k9_golden():
    from pn2 import F32
    from pn2.engine import Engine, Act
    from pn2.graph import _seed_grad
    z = np.load(os.path.join(G, "dsra_k9.npz"))
    for sm, tag in ((True, "sm"), (False, "nosm")):
        eng = Engine(F32, True, need_grad=True)
        mk = lambda k: Act(eng, torch.from_numpy(z[k]).to(dev).permute(0, 2, 3, 1).contiguous(), 9, 9, 9, F32)
        fg, cf, cb = mk("fg"), mk("crop_fg"), mk("crop_bg")
        y = eng.dsra_fuse(fg, cf, cb, sm)
        _seed_grad(y, torch.from_numpy(z["gout"]).to(dev)); eng.backward()
        assert relmax(y.t.permute(0, 3, 1, 2), torch.from_numpy(z[tag + "_y"])) < 1e-5
        for a, k in ((fg, "gfg"), (cf, "gcf"), (cb, "gcb")):
            assert relmax(a.grad.permute(0, 3, 1, 2), torch.from_numpy(z[f"{tag}_{k}"])) < 1e-5


@pytest.mark.parametrize("skip", [True, False])
def test_dsra_k1_degenerates_to_doubling(skip, monkeypatch):
    """num_class=1: softmax over one channel is 1.0, so fg <- 2*fg and d/dcrop == 0 exactly (SURVEY 'three facts' #2).  The engine uses that:
    the crop maps receive NO gradient contribution (ZERO_CROP_SKIP), so the resamples that produced them skip their adjoints; with the switch off
    the kernel writes the (exactly zero) crop gradients."""
    from pn2 import F32, engine, core
    from pn2.engine import Engine, Act
    from pn2.graph import _seed_grad
    monkeypatch.setattr(core, "ZERO_CROP_SKIP", skip)
    eng = Engine(F32, True, need_grad=True)
    mk = lambda: Act(eng, torch.randn(2, 7, 7, 1, device=dev), 1, 1, 1, F32)
    fg, src_f, src_b = mk(), Act(eng, torch.randn(2, 14, 14, 1, device=dev), 1, 1, 1, F32), mk()
    cf = eng.bilinear(src_f, 0.5)               # a crop made by a resample, as in pranet.py:353
    y = eng.dsra_fuse(fg, cf, src_b, True)
    gy = torch.randn(2, 1, 7, 7, device=dev)
    _seed_grad(y, gy); eng.backward()
    assert torch.equal(y.t, 2 * fg.t)
    assert torch.equal(fg.grad, 2 * gy.permute(0, 2, 3, 1))
    for a in (cf, src_b, src_f):
        assert (a.grad is None or not a.grad_written) if skip else float(a.grad.abs().max()) == 0.0


@pytest.mark.parametrize("tag", ["rand", "zeros", "ones"])
def test_structure_loss_golden(tag):
    from pn2.loss import structure_loss
    z = np.load(os.path.join(G, "structure_loss.npz"))
    pred = torch.from_numpy(z[f"{tag}_pred"]).to(dev).requires_grad_(True)
    pbg = torch.from_numpy(z[f"{tag}_pred_bg"]).to(dev).requires_grad_(True)
    mask = torch.from_numpy(z[f"{tag}_mask"]).to(dev)
    loss = structure_loss(pred, pbg, mask, 1 - mask)
    loss.backward()
    assert abs(float(loss) - float(z[f"{tag}_loss"])) < 2e-6
    assert relmax(pred.grad, torch.from_numpy(z[f"{tag}_gpred"])) < 2e-5
    assert relmax(pbg.grad, torch.from_numpy(z[f"{tag}_gpred_bg"])) < 2e-5


def _module_vs_oracle(mod, oracle_fn, inputs, dtn):
    import pn2
    from oracle import pranet_oracle as O
    pn2.set_compute_dtype(dtn)
    err, tol = (relmax, 5e-5) if dtn == "fp32" else (rell2, 8e-2)
    mod = mod.to(dev).train()
    P = {k: v.detach().cpu().clone() for k, v in mod.state_dict().items()}
    xs = [x.to(dev).requires_grad_(True) for x in inputs]
    outs = mod(*xs)
    outs = outs if isinstance(outs, (tuple, list)) else (outs,)
    torch.manual_seed(5)
    gs = [torch.randn_like(o) for o in outs]
    torch.autograd.backward(list(outs), gs)
    keys = O.params_of(P)
    for k in keys:
        P[k].requires_grad_(True)
    xc = [x.detach().cpu().requires_grad_(True) for x in inputs]
    ro = oracle_fn(P, *xc)
    ro = ro if isinstance(ro, (tuple, list)) else (ro,)
    torch.autograd.backward(list(ro), [g.cpu() for g in gs])
    for o, r in zip(outs, ro):
        assert err(o, r) < tol
    for x, c in zip(xs, xc):
        assert err(x.grad, c.grad) < tol
    named = dict(mod.named_parameters())
    # Every parameter gradient keeps the per-tensor bound tol * 5 (bf16: measured <= 0.16 on the 1-D BatchNorm vectors, <= 0.1 on conv weights).  ONE vector
    # is named as an exception: bns.2.bias of a Bottle2neck, the bias gradient of the deepest branch - 4..16 numbers, each a CANCELLING sum of ReLU-masked
    # dy over a few hundred pixels of this small block; one element whose normalised value sits next to 0 flips its mask under any change in the order of
    # bf16 roundings and moves the sum by |dy| (measured 0.03 / 0.16 / 0.43 on the three blocks, tools/probe_gates.py).  It gets < 1.0 and is covered by the
    # pooled bound over all 1-D gradients of the block.
    UNSTABLE_BF16 = ("bns.2.bias",)
    pool_a, pool_b = [], []
    for k in keys:
        if P[k].grad is not None:
            e = err(named[k].grad, P[k].grad)
            if os.environ.get("PN2_TEST_VERBOSE"):
                print(f"   grad {k:28s} err {e:.3e}")
            if dtn != "fp32" and P[k].ndim == 1:
                pool_a.append(named[k].grad.detach().reshape(-1).cpu().double()); pool_b.append(P[k].grad.reshape(-1).double())
            assert e < (1.0 if (dtn != "fp32" and k in UNSTABLE_BF16) else tol * 5), (k, e)
    if pool_a:
        assert err(torch.cat(pool_a), torch.cat(pool_b)) < tol * 5
    sd = mod.state_dict()
    for k in sd:
        if "running" in k:
            assert err(sd[k].float(), P[k].detach().float()) < tol, k
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(P[k])


def _rnd(m, seed=3):
    g = torch.Generator().manual_seed(seed)
    for p in m.parameters():
        p.data = torch.randn(p.shape, generator=g) * (0.2 if p.ndim > 1 else 0.3) + (1.0 if p.ndim == 1 else 0.0)
    return m


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
def test_blocks_vs_oracle(dtn):
    from lib.Res2Net_v1b import Bottle2neck
    from lib.pranet import RFB_modified, aggregation
    from oracle import pranet_oracle as O
    g = torch.Generator().manual_seed(4)
    r = lambda *s: torch.randn(*s, generator=g)
    _module_vs_oracle(_rnd(Bottle2neck(64, 16)), lambda P, x: O.bottle2neck(P, "", x, O.Ctx(True), 1, False, False), [r(2, 64, 12, 12)], dtn)
    _module_vs_oracle(_rnd(Bottle2neck(256, 64)), lambda P, x: O.bottle2neck(P, "", x, O.Ctx(True), 1, False, False), [r(2, 256, 10, 10)], dtn)
    down = nn.Sequential(nn.AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False), nn.Conv2d(64, 128, 1, bias=False), nn.BatchNorm2d(128))
    _module_vs_oracle(_rnd(Bottle2neck(64, 32, stride=2, downsample=down, stype="stage")), lambda P, x: O.bottle2neck(P, "", x, O.Ctx(True), 2, True, True), [r(2, 64, 13, 13)], dtn)
    _module_vs_oracle(_rnd(RFB_modified(48, 32)), lambda P, x: O.rfb(P, "", x, O.Ctx(True)), [r(2, 48, 11, 11)], dtn)
    _module_vs_oracle(_rnd(aggregation(32, 1)), lambda P, a, b, c: O.aggregation(P, "", a, b, c, O.Ctx(True)), [r(2, 32, 3, 3), r(2, 32, 6, 6), r(2, 32, 12, 12)], dtn)


def test_blocks_golden_fp32():
    """Bottle2neck / RFB / aggregation against vectors produced by the reference's own classes (tests/golden/blocks.npz)."""
    import pn2
    from lib.Res2Net_v1b import Bottle2neck
    from lib.pranet import RFB_modified, aggregation
    pn2.set_compute_dtype("fp32")
    z = np.load(os.path.join(G, "blocks.npz"))

    def load(mod, prefix):
        sd = {}
        for k in z.files:
            if k.startswith(prefix):
                n = k[len(prefix):]; v = torch.from_numpy(z[k]).clone()
                if n.endswith("running_mean"): v.zero_()
                if n.endswith("running_var"): v.fill_(1.0)
                if n.endswith("num_batches_tracked"): v.zero_()
                sd[n] = v
        mod.load_state_dict(sd, strict=True)
        return mod.to(dev).train()
    T = lambda k: torch.from_numpy(z[k]).to(dev)
    b = load(Bottle2neck(64, 16), "b2n_sd.")
    assert relmax(b(T("b2n_x")), T("b2n_y")) < 5e-5
    for k, v in b.state_dict().items():
        assert relmax(v.float(), T("b2n_sd." + k).float()) < 5e-5, k
    down = nn.Sequential(nn.AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False), nn.Conv2d(64, 128, 1, bias=False), nn.BatchNorm2d(128))
    b = load(Bottle2neck(64, 32, stride=2, downsample=down, stype="stage"), "b2s_sd.")
    assert relmax(b(T("b2s_x")), T("b2s_y")) < 5e-5
    r = load(RFB_modified(48, 32), "rfb_sd.")
    assert relmax(r(T("rfb_x")), T("rfb_y")) < 5e-5
    a = load(aggregation(32, 1), "agg_sd.")
    fg, bg = a(T("agg_x1"), T("agg_x2"), T("agg_x3"))
    assert relmax(fg, T("agg_fg")) < 5e-4 and relmax(bg, T("agg_bg")) < 5e-4


def _fixture_model(fp32=True):
    import pn2
    from lib.pranet import PraNet_V2
    from oracle import weights as W
    pn2.set_compute_dtype(fp32 if isinstance(fp32, str) else ("fp32" if fp32 else "bf16"))          # (or a mode name: "fp32fast")
    model = PraNet_V2(num_class=1)
    model.load_state_dict(W.make_state_dict(W.manifest_pranet_v2(1), seed=0), strict=True)
    return model.to(dev).train()


@pytest.mark.parametrize("tag", ["96", "352"])
def test_model_forward_backward_vs_reference(tag):
    """nn.Module surface + torch autograd (the MyTrain_med.py:76-84 path) against the imported reference's vectors."""
    from pn2.loss import structure_loss
    from oracle import weights as W
    z = np.load(os.path.join(G, f"pranet_v2_{tag}.npz"))
    size, n = int(z["size"]), int(z["n"])
    model = _fixture_model()
    x, mask = W.synthetic_batch(n, size, seed=1234)
    x, mask = x.to(dev), mask.to(dev)
    outs = model(x)
    assert len(outs) == 8 and all(o.shape == (n, 1, size, size) for o in outs)
    losses = [structure_loss(outs[i], outs[i + 4], mask, 1 - mask) for i in range(4)]          # MyTrain_med.py:78-81
    loss = losses[3] + losses[2] + losses[1] + losses[0]
    loss.backward()
    own_l = float(np.abs(z["s1.losses"] - z["f64.losses"]).max())
    assert max(abs(float(l.detach()) - float(r)) for l, r in zip(losses, z["f64.losses"])) < max(1e-5, 0.6 * own_l)
    full = tag == "96"
    for i, o in enumerate(outs):
        r32 = torch.from_numpy(z[f"s1.out{i}"]).double(); r64 = torch.from_numpy(z[f"f64.out{i}"])
        got = (o.detach().cpu() if full else o.detach().cpu()[:, :, ::4, ::4]).double()
        own = float((r32 - r64).abs().max())
        e = float((got - r64).abs().max())
        assert e <= max(1e-4, 0.6 * own), (i, e, own)          # measured 0.25-0.4 x own (tests/parity_probe.py)
    named = dict(model.named_parameters())
    rows = []
    for f in z.files:
        if f.startswith("graw."):
            k = f[5:]
            r32 = torch.from_numpy(z[f]).double(); r64 = torch.from_numpy(z["f64." + f]).double()
            got = named[k].grad.reshape(-1)[:256].cpu().double()
            own = float((r32 - r64).norm() / (r64.norm() + 1e-30))
            e = float((got - r64).norm() / (r64.norm() + 1e-30))
            rows.append((k, e, own))
    # gradients through ~60 train-mode BN layers are ill-conditioned (the reference's own fp32 error reaches 4e-2 on the stem), and an fp32 gradient of
    # a ReLU network is only piecewise continuous: an element within rounding of zero takes the other branch than in float64 and shifts every
    # gradient upstream of it (tests/test_gpu_cond.py).  Gates: EVERY probe at least as close to the float64 gradient as the reference's own fp32 gradient is
    # (ratio <= 1.0; measured 0.23-0.64 on both fixtures, tools/probe_gates.py), and the typical probe clearly closer (median <= 0.8).  ONE probe is a named
    # exception: layer4.0.convs.1.weight at 96^2, a 3x3 stride-2 conv whose output has 2 x 3 x 3 = 18 pixels per channel in front of a train-mode BatchNorm
    # (measured 1.17 x the reference's own error; allowed 2 x).
    OUTLIERS = {("96", "backbone.layer4.0.convs.1.weight"): 2.0}
    ratios = sorted(e / max(own, 2.5e-6) for _k, e, own in rows)
    bad = [r for r in rows if r[1] > max(2e-6, OUTLIERS.get((tag, r[0]), 1.0) * r[2])]
    assert ratios[len(ratios) // 2] <= 0.8 and not bad, (ratios[len(ratios) // 2], bad)
    no_grad = sorted(k for k, p in named.items() if p.grad is None)
    assert no_grad == sorted(str(s) for s in z["nograd"])


VARIANTS = {"k3": (dict(), "v2", 0, 1234), "k3lin": (dict(num_class=3, use_softmax=False, sem_downsample=2), "v2", 0, 1234), "pvtk3": (dict(num_class=3), "pvt", 3, 4321)}


@pytest.mark.parametrize("tag", sorted(VARIANTS))
def test_constructor_variants_vs_reference(tag):
    """The constructor paths the binary scripts never take, end to end through the nn.Module surface + torch autograd on the fp32 path, against the
    reference's own classes (tests/golden/make_golden_variants.py): PraNet_V2() with its DEFAULT arguments (num_class=3: the DSRA softmax is not the
    identity, pranet.py:270,365-368), PraNet_V2(num_class=3, use_softmax=False, sem_downsample=2) (linear fusion, half-resolution maps, :349-350) and
    PVT_PraNet_V2(num_class=3).  Backward under fixed cotangents (structure_loss is a one-channel loss).  Gates: every map within
    max(1e-4, 1.0 x |ref32 - ref64|) of the float64 run - no further from the exact result than the reference's own fp32 run (measured 0.3-0.65 x;
    PVT, whose own gap is 3e-5: 3 x), every gradient probe at least as close to the
    float64 gradient as the reference's own fp32 gradient."""
    import pn2
    from lib.pranet import PraNet_V2, PVT_PraNet_V2
    from oracle import weights as W
    pn2.set_compute_dtype("fp32")
    z = np.load(os.path.join(G, "pranet_v2_variants.npz"))
    kw, fam, wseed, xseed = VARIANTS[tag]
    model = (PraNet_V2 if fam == "v2" else PVT_PraNet_V2)(**kw)
    if fam == "pvt":
        model.backbone.reset_drop_path(0.0)
    model.load_state_dict(W.make_state_dict(W.manifest_pranet_v2(3) if fam == "v2" else W.manifest_pvt_pranet_v2(3), seed=wseed), strict=True)
    model = model.to(dev).train()
    x, _ = W.synthetic_batch(2, 96, seed=xseed)
    outs = model(x.to(dev))
    assert len(outs) == 8 and all(tuple(o.shape) == tuple(int(v) for v in z[f"{tag}.shape"]) for o in outs)
    g = torch.Generator().manual_seed(99)
    gs = [torch.randn(o.shape, generator=g) for o in outs]
    sum((o * c.to(dev)).sum() for o, c in zip(outs, gs)).backward()
    k_own = 1.0 if fam == "v2" else 3.0
    rows = []
    for i, o in enumerate(outs):
        r64 = torch.from_numpy(z[f"{tag}.f64.out{i}"])
        rows.append((i, float((o.detach().cpu().double()[:, :, ::2, ::2] - r64).abs().max()), float(z[f"{tag}.own_abs"][i])))
    if os.environ.get("PN2_TEST_VERBOSE"):
        print(tag, [(i, f"{e:.2e}", f"{own:.2e}") for i, e, own in rows])
    assert all(e <= max(1e-4, k_own * own) for _i, e, own in rows), (tag, rows)
    named = dict(model.named_parameters())
    bad = []
    for f in z.files:
        if f.startswith(f"{tag}.f64.graw."):
            k = f[len(f"{tag}.f64.graw."):]
            r64 = torch.from_numpy(z[f]).double(); r32 = torch.from_numpy(z[f"{tag}.graw.{k}"]).double()
            got = named[k].grad.reshape(-1)[:256].cpu().double()
            own = float((r32 - r64).norm() / (r64.norm() + 1e-30)); e = float((got - r64).norm() / (r64.norm() + 1e-30))
            if e > max(2e-5 if fam == "pvt" else 2e-6, 1.0 * own):
                bad.append((k, e, own))
    assert not bad, bad
    assert sorted(k for k, p in named.items() if p.grad is None) == sorted(str(s_) for s_ in z[f"{tag}.nograd"])
    sd = model.state_dict()
    for f in z.files:
        if f.startswith(f"{tag}.buf."):
            k = f[len(f"{tag}.buf."):]
            assert relmax(sd[k].reshape(-1)[:256].float(), torch.from_numpy(z[f])) < 1e-4, k


@pytest.mark.parametrize("tag", ["96", "352"])
def test_model_bf16_vs_reference_f64(tag, monkeypatch):
    """The BENCHMARKED precision (bf16 storage + bf16 MFMA, fp32 accumulate) end to end against the float64 run of the imported reference.
    These fixtures (random init, train-mode BN over 2 images) amplify rounding noise ~500x from the stem to the logits, so every bf16
    execution sits O(1) relative L2 away from the float64 maps; the yardstick is the imported reference under PyTorch's own bf16 policy
    (torch.autocast("cpu", bfloat16): tests/golden/make_golden_bf16.py).  Gates, per map: rel-L2(ours, ref64) <= 1.5 x rel-L2(torch bf16, ref64);
    pair losses within 10 % (torch's own bf16 run: 4.6 %); meanDic of the MyTest_med.py:104-111 map no further from the float64 value
    than torch's bf16 map is (+5e-2: the fixture's meanDic is 0.07, i.e. noise).  'Dice within 1e-3' itself is a property of the fp32 path (test_eval_tail_and_dice_on_train_mode_logits)."""
    from pn2.loss import structure_loss
    from pn2.evaltail import test_postprocess
    from oracle import weights as W
    from oracle import pranet_oracle as O
    z = np.load(os.path.join(G, f"pranet_v2_{tag}.npz"))
    zb = np.load(os.path.join(G, "pranet_v2_bf16ref.npz"))
    size, n = int(z["size"]), int(z["n"])
    # heuristic tiles: the tuner's choice depends on what it timed (and on the tests that ran before), the tile size decides how the BatchNorm partial
    # statistics are grouped, and this fixture amplifies a last-bit difference ~500x - with the tuner on the numbers below move from run to run
    monkeypatch.setenv("PN2_AUTOTUNE", "0")
    model = _fixture_model(fp32=False)
    x, mask = W.synthetic_batch(n, size, seed=1234)
    xg, mg = x.to(dev), mask.to(dev)
    with torch.no_grad():
        outs = model(xg)
    full = tag == "96"
    errs, torch_errs = [], []
    for i, o in enumerate(outs):
        r64 = torch.from_numpy(z[f"f64.out{i}"])
        got = (o.cpu() if full else o.cpu()[:, :, ::4, ::4]).double()
        errs.append(rell2(got, r64)); torch_errs.append(rell2(torch.from_numpy(zb[f"{tag}.out{i}"]), r64))
    losses = [float(structure_loss(outs[i], outs[i + 4], mg, 1 - mg)) for i in range(4)]
    lerr = [abs(l - float(r)) / abs(float(r)) for l, r in zip(losses, z["f64.losses"])]
    tlerr = [abs(float(l) - float(r)) / abs(float(r)) for l, r in zip(zb[f"{tag}.losses"], z["f64.losses"])]
    print(f"bf16 vs f64 [{tag}]: rel-L2 per map ours {[f'{e:.2f}' for e in errs]}  torch-bf16 {[f'{e:.2f}' for e in torch_errs]}")
    print(f"   rel loss err ours {[f'{e:.1e}' for e in lerr]}  torch-bf16 {[f'{e:.1e}' for e in tlerr]}")
    for e, t in zip(errs, torch_errs):
        assert e <= 1.5 * t, (errs, torch_errs)              # two realisations of amplified rounding noise: measured 0.85 .. 1.4 x torch's
    for e, t in zip(lerr, tlerr):
        assert e <= 1e-1, (lerr, tlerr)                      # measured <= 6.9e-2 (torch's own bf16: <= 4.6e-2)
    if full:
        dice_gate = []
        for shape in ((104, 90), (96, 96)):
            gt = torch.nn.functional.interpolate(mask[:1], size=shape, mode="nearest")[0, 0].numpy()
            ours = test_postprocess([o[:1] for o in outs], shape).cpu().numpy()
            ref = O.test_postprocess([torch.from_numpy(z[f"f64.out{i}"])[:1].float() for i in range(8)], shape)
            tb = O.test_postprocess([torch.from_numpy(zb[f"{tag}.out{i}"])[:1] for i in range(8)], shape)
            d_ours, d_torch = abs(O.mean_dice(ours, gt) - O.mean_dice(ref, gt)), abs(O.mean_dice(tb, gt) - O.mean_dice(ref, gt))
            print(f"   meanDic f64 {O.mean_dice(ref, gt):.5f}: ours-bf16 off by {d_ours:.1e}, torch-bf16 off by {d_torch:.1e}")
            dice_gate.append((d_ours, d_torch))
        assert all(a <= b + 5e-2 for a, b in dice_gate), dice_gate          # meanDic of this random-init fixture is 0.07: noise on noise (measured 0.08 vs torch's 0.05)


def test_bf16_training_trajectory_vs_fp32_oracle():
    """20 MyTrain_med.py steps (lr 1e-4, clip 0.5) on one fixed batch: the bf16 fused trainer against the CPU oracle in fp32.  The loss
    curves must stay together (bf16 noise does not accumulate into a different trajectory) and the loss must fall."""
    from pn2.trainer import Trainer
    from oracle import weights as W
    from oracle import pranet_oracle as O
    model = _fixture_model(fp32=False)
    x, mask = W.synthetic_batch(2, 96, seed=1234)
    xg, mg = x.to(dev), mask.to(dev)
    tr = Trainer(model, lr=1e-4, clip=0.5)
    NS = 20
    ours = [float(tr.step(xg, mg)[-1]) for _ in range(NS)]
    P = W.make_state_dict(W.manifest_pranet_v2(1), seed=0)
    st = {}
    ref = [float(O.train_step(P, st, x, mask)[0]) for _ in range(NS)]
    rel = [abs(a - b) / b for a, b in zip(ours, ref)]
    print("bf16 trajectory:", [f"{v:.4f}" for v in ours[::4]], " oracle fp32:", [f"{v:.4f}" for v in ref[::4]], f" max rel diff {max(rel):.2e}, last {rel[-1]:.2e}")
    # measured over 20 steps: <= 2.7 % .. 5.3 % on single steps depending on the tiles the tuner picked (the first Adam steps move every weight by
    # ~lr * sign(g), see the 2-step test), 0.75 % .. 2 % at the end; loss 9.39 -> 5.88 (oracle 9.55 -> 5.85)
    assert max(rel) < 8e-2 and rel[-1] < 4e-2, rel
    assert ours[-1] < 0.9 * ours[0] and ref[-1] < 0.9 * ref[0]


def test_trainer_two_steps_and_eval_tail_vs_reference():
    """Fused trainer (flat arenas, fused 4-pair loss, clamp+Adam kernel): two MyTrain_med.py steps, then MyTest_med.py eval + tail."""
    from pn2.trainer import Trainer
    from pn2.evaltail import test_postprocess
    from oracle import weights as W
    from oracle import pranet_oracle as O
    z = np.load(os.path.join(G, "pranet_v2_96.npz"))
    model = _fixture_model()
    x, mask = W.synthetic_batch(2, 96, seed=1234)
    xg, mg = x.to(dev), mask.to(dev)
    tr = Trainer(model, lr=1e-4, clip=0.5)
    named = dict(model.named_parameters()); bufs = dict(model.named_buffers())
    for step in (1, 2):
        loss = tr.step(xg, mg)
        s = f"s{step}."
        # step 1 sees identical weights; step 2 follows one Adam update, which at t=1 moves every weight by ~lr*sign(g): sign flips
        # of noise-level gradients make the step-2 loss differ at the 1e-3 level between ANY two fp32 implementations
        ltol = 2e-4 if step == 1 else 3e-2
        assert abs(float(loss[-1]) - float(z[s + "loss"])) < ltol
        assert np.abs(loss[:4].cpu().numpy() - z[s + "losses"]).max() < ltol
        for k in [f[len(s + "param."):] for f in z.files if f.startswith(s + "param.")]:
            assert float((named[k].detach().reshape(-1)[:256].cpu() - torch.from_numpy(z[s + "param." + k])).abs().max()) < 2.1e-4 * step, k
        for k in [f[len(s + "buf."):] for f in z.files if f.startswith(s + "buf.")]:
            ref = torch.from_numpy(z[s + "buf." + k])
            btol = 1e-4 if step == 1 else 1e-2       # step 2 statistics see weights after a sign-like Adam update (see above)
            assert float((bufs[k].reshape(-1)[:256].cpu() - ref).abs().max()) < btol * max(1.0, float(ref.abs().max())), k
    assert int(bufs["backbone.bn1.num_batches_tracked"]) == 2
    # Adam moves every coordinate by <= lr per step; most probes must agree far better than that bound
    k = "ra2_conv4_fg.conv.weight"
    d = (named[k].detach().reshape(-1)[:256].cpu() - torch.from_numpy(z["s2.param." + k])).abs()
    assert float(d.median()) < 1e-6 and float(d.quantile(0.9)) < 2e-5 and float(d.max()) < 4.2e-4
    # ---- eval forward (running statistics) + MyTest_med.py tail
    model.eval()
    with torch.no_grad():
        outs = model(xg[:1])
    for i, o in enumerate(outs):
        ref = torch.from_numpy(z[f"eval.out{i}"])
        # two momentum-0.1 updates leave the running statistics far from the batch statistics, so eval-mode logits reach
        # ~1e7 here (SURVEY §7 'hard parts'); only a loose relative bound is meaningful for them
        assert float((o.cpu() - ref).abs().max()) < 0.1 * max(1.0, float(ref.abs().max())), i
    u8 = test_postprocess(outs, z["eval.u8"].shape).cpu().numpy()
    assert u8.shape == z["eval.u8"].shape
    # with logits ~1e7 the sigmoid saturates and the map is a hard sign pattern: pixels flip on rounding noise, so this
    # fixture only supports a loose agreement check; the strict Dice bound is tested below on O(1) logits
    assert np.mean(np.abs(u8.astype(int) - z["eval.u8"].astype(int)) <= 2) > 0.9
    assert abs(O.mean_dice(u8, z["eval.gt"]) - float(z["eval.meanDic"])) < 2e-2


def test_eval_tail_and_dice_on_train_mode_logits():
    """MyTest_med.py:104-111 tail + meanDic (eval.py:22,44-50) on well-conditioned (O(1)) logits: ours vs the tail applied to
    the reference's own step-1 outputs.  'Dice within 1e-3' (BASELINE.json north_star)."""
    from pn2.evaltail import test_postprocess
    from oracle import weights as W
    from oracle import pranet_oracle as O
    z = np.load(os.path.join(G, "pranet_v2_96.npz"))
    model = _fixture_model()
    x, mask = W.synthetic_batch(2, 96, seed=1234)
    with torch.no_grad():
        outs = model(x.to(dev))                       # train-mode BN (batch statistics), no autograd
    gt = torch.nn.functional.interpolate(mask[:1], size=(104, 90), mode="nearest")[0, 0].numpy()
    ours = test_postprocess([o[:1] for o in outs], (104, 90)).cpu().numpy()
    ref = O.test_postprocess([torch.from_numpy(z[f"s1.out{i}"])[:1] for i in range(8)], (104, 90))
    assert np.abs(ours.astype(int) - ref.astype(int)).max() <= 1
    assert abs(O.mean_dice(ours, gt) - O.mean_dice(ref, gt)) < 1e-3


def test_threshold_metrics_vs_reference_and_oracle():
    """GPU histogram sweep == the imported reference's Fmeasure_calu curves (golden) bit for bit, and == the oracle at 352x352."""
    from pn2.evaltail import threshold_metrics
    from oracle import pranet_oracle as O
    z = np.load(os.path.join(G, "eval_metrics.npz"))
    for tag in ("blob", "zero_pred", "zero_gt", "exact", "full"):
        r = threshold_metrics(torch.from_numpy(z[tag + "_pred"]).to(dev), torch.from_numpy(z[tag + "_gt"]).to(dev))
        assert np.array_equal(r["curves"], z[tag + "_curves"], equal_nan=True), tag
        assert abs(r["mae"] - float(z[tag + "_mae"])) < 1e-12
        if tag != "full":
            assert r["meanDic"] == float(z[tag + "_means"][3]) and r["meanIoU"] == float(z[tag + "_means"][5])
    rng = np.random.default_rng(11)
    pred = rng.integers(0, 256, (352, 352), dtype=np.uint8)
    gt = (rng.random((352, 352)) < 0.2).astype(np.float32)
    r = threshold_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev))
    cols, mae = O.threshold_metrics(pred, gt)
    assert np.array_equal(r["curves"], cols) and abs(r["mae"] - mae) < 1e-12
    assert abs(r["meanDic"] - O.mean_dice(pred, gt)) < 1e-12


def test_full_eval_metrics_vs_reference_eval_for_testAllInOne():
    """Sm, wFm and meanEm on the device (pn2_eval_region_sums, pn2_eval_wfm + the histograms) against the imported reference's eval_for_testAllInOne
    (eval.py:18-66; tests/golden/make_golden_evalfull.py): every metric of opt["metrics"] within 1e-9 (the reference sums pixels pairwise in float64, the device
    path uses exact integer moments / fixed-order sums), the EnhancedMeasure threshold curve within 1e-12, and - through the C ABI - the exact Euclidean feature
    transform: distances and the error propagated from the nearest foreground pixel IDENTICAL to scipy's on a map full of equidistant sites."""
    import ctypes as C
    import warnings
    from pn2.evaltail import threshold_metrics, eval_for_testAllInOne
    from pn2.capi import call
    from oracle import pranet_oracle as O
    z = np.load(os.path.join(G, "eval_full.npz"))
    names = ["meanDic", "meanIoU", "wFm", "Sm", "meanEm", "mae"]
    for tag in ("blob", "zero_pred", "exact", "full", "two", "rand352"):
        pred, gt = torch.from_numpy(z[tag + "_pred"]).to(dev), torch.from_numpy(z[tag + "_gt"]).to(dev)
        r = threshold_metrics(pred, gt, full=True)
        for k, ref in zip(names, z[tag + "_vals"]):
            assert abs(r[k] - float(ref)) <= 1e-9 * max(1.0, abs(float(ref))), (tag, k, r[k], float(ref))
        assert np.abs(r["E"] - z[tag + "_E"]).max() <= 1e-12, tag
        assert eval_for_testAllInOne({"metrics": ["Sm", "mae", "wFm"]}, pred, gt) == [r["Sm"], r["mae"], r["wFm"]]
    # no foreground at all: Sm = 1 - mean(pred) (eval_functions.py:79-81), meanEm from 1 - pred; wFm is undefined in the reference (scipy has no site to return)
    pred = torch.from_numpy(z["blob_pred"]).to(dev)
    r = threshold_metrics(pred, torch.zeros_like(pred, dtype=torch.float32), full=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        o = O.full_metrics(z["blob_pred"], np.zeros_like(z["blob_gt"]))
    assert abs(r["Sm"] - o["Sm"]) < 1e-12 and abs(r["meanEm"] - o["meanEm"]) < 1e-12 and np.isnan(r["wFm"])
    # ---- the feature transform itself, through the C ABI
    P = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    K = torch.full((49,), 1.0 / 49, dtype=torch.float64, device=dev)
    for gt_np, pred_np in ((z["tie_gt"], None), (z["blob_gt"], z["blob_pred"])):
        H, W = gt_np.shape
        gt = torch.from_numpy(gt_np).to(dev)
        pred = torch.from_numpy(pred_np).to(dev) if pred_np is not None else torch.zeros(H, W, dtype=torch.uint8, device=dev)
        wi = torch.empty(H * W, dtype=torch.int32, device=dev); wd = torch.empty(2 * H * W, dtype=torch.float64, device=dev)
        part = torch.empty(int(call.pn2_eval_wfm_blocks(H, W)), 2, dtype=torch.float64, device=dev)
        call.pn2_eval_wfm(P(pred), P(gt), H, W, P(K), -0.1, P(wi), P(wd), P(part), st)
        torch.cuda.synchronize()
        et, dst = wd[:H * W].reshape(H, W).cpu().numpy(), wd[H * W:].reshape(H, W).cpu().numpy()
        if pred_np is None:
            assert np.array_equal(dst, z["tie_dst"])
            # with pred = 0 the propagated error is 1 everywhere (|0 - 1| at a foreground pixel): use the distances only here, the indices via the blob case below
            assert np.array_equal(et, np.ones_like(et))
        else:
            assert np.array_equal(et, z["blob_Et"])


@pytest.mark.parametrize("which", ["res2net", "pvt"])
def test_v1_forward_vs_reference(which):
    """PraNet / PVT_PraNet (V1 reverse attention, PraNet_Res2Net.py:101-273; the two V1 models MyTest_med.py:58-66 loads strict) in fp32
    against the imported reference run in float64: outputs and gradient probes must be closer to it than the reference's own fp32 run
    (same gate as test_model_forward_backward_vs_reference)."""
    import pn2
    from lib.PraNet_Res2Net import PraNet, PVT_PraNet
    from oracle import weights as W
    pn2.set_compute_dtype("fp32")
    if which == "res2net":
        z = np.load(os.path.join(G, "pranet_v1_96.npz"))
        model = PraNet()
        model.load_state_dict(W.make_state_dict(W.manifest_pranet_v1(), seed=1), strict=True)
        x, _ = W.synthetic_batch(2, 96, seed=77)
    else:
        z = np.load(os.path.join(G, "pvt_pranet_v1_96.npz"))
        model = PVT_PraNet()
        model.load_state_dict(W.make_state_dict(W.manifest_pvt_pranet_v1(), seed=7), strict=True)
        model.backbone.reset_drop_path(0.0)
        x, _ = W.synthetic_batch(2, 96, seed=78)
    model = model.to(dev).train()
    outs = model(x.to(dev))
    assert len(outs) == 4 and all(o.shape == (2, 1, 96, 96) for o in outs)          # (lateral_map_5, 4, 3, 2)
    loss = sum(o.square().mean() for o in outs)
    loss.backward()
    for i, o in enumerate(outs):
        r32 = torch.from_numpy(z[f"out{i}"]).double(); r64 = torch.from_numpy(z[f"f64.out{i}"]).double()
        own = float((r32 - r64).abs().max()); e = float((o.detach().cpu().double() - r64).abs().max())
        assert e <= max(1e-4, 0.8 * own), (i, e, own)
    named = dict(model.named_parameters())
    for f in z.files:
        if f.startswith("graw."):
            k = f[5:]
            r32 = torch.from_numpy(z[f]).double(); r64 = torch.from_numpy(z["f64." + f]).double()
            own = rell2(r32, r64); e = rell2(named[k].grad.reshape(-1)[:256], r64)
            assert e <= max(2e-6, 1.1 * own), (k, e, own)          # measured <= 1.03 x the reference's own fp32 error (the gate / sigmoid kernels use the hardware exp)


def test_graph_replay_matches_eager_bf16():
    from pn2.trainer import Trainer
    from oracle import weights as W
    x, mask = W.synthetic_batch(2, 96, seed=9)
    xg, mg = x.to(dev), mask.to(dev)
    res = []
    for graph in (False, True):
        model = _fixture_model(fp32=False)
        tr = Trainer(model, lr=1e-4, clip=0.5)
        if graph:
            tr.capture(xg, mg, warmup=2)
            for _ in range(2):
                loss = tr.replay()
        else:
            for _ in range(4):
                loss = tr.step(xg, mg)
        torch.cuda.synchronize()
        res.append((loss.clone(), tr.flat.clone()))
    assert torch.allclose(res[0][0], res[1][0], rtol=0, atol=0), "hipGraph replay must be bit-identical to eager launches"
    assert torch.equal(res[0][1], res[1][1])


def test_lr_schedule_reaches_captured_graph():
    """utils.adjust_lr (MyTrain_med.py:155) on the fused trainer: the optimizer kernel reads lr from the device, so a captured hipGraph follows
    the schedule without a re-capture (the by-value lr used to be baked into the graph)."""
    from pn2.trainer import Trainer
    from utils.utils import adjust_lr
    from oracle import weights as W
    x, m = W.synthetic_batch(2, 96, seed=9)
    xg, mg = x.to(dev), m.to(dev)
    tr = Trainer(_fixture_model(fp32=False), lr=1e-4, clip=0.5)
    tr.capture(xg, mg, warmup=2)
    p0 = tr.flat.clone(); tr.replay(); torch.cuda.synchronize()
    d1 = float((tr.flat - p0).abs().max())
    assert 0.5e-4 < d1 <= 1.01e-4 * 3.2                       # Adam: |step| <= lr * (1 - b1^t) / sqrt(1 - b2^t) ~ lr early on
    adjust_lr(tr, 1e-4, epoch=60, decay_rate=0.1, decay_epoch=30)          # lr *= 0.1 ** 2
    assert abs(tr.lr - 1e-6) < 1e-12
    p1 = tr.flat.clone(); tr.replay(); torch.cuda.synchronize()
    d2 = float((tr.flat - p1).abs().max())
    assert d2 < 0.02 * d1 and d2 > 0
    tr.set_lr(0.0)
    p2 = tr.flat.clone(); tr.replay(); torch.cuda.synchronize()
    assert torch.equal(tr.flat, p2)


@pytest.mark.parametrize("fp32", [False, True, "fp32fast"])
def test_table_driven_launches_match_single_launches(fp32, monkeypatch):
    """pn2_conv_wgrad_multi / pn2_wgrad_reduce_multi over the step arena == one pn2_conv_wgrad + pn2_wgrad_reduce per conv, bit for bit."""
    from pn2 import core
    from pn2.trainer import Trainer
    from oracle import weights as W
    monkeypatch.setattr(core, "WGRAD_SLAB_CAP", 0.0)       # same pixel splits in both forms (the table form otherwise runs fewer: GradQueue.table_splits, tests/test_gpu_switches.py)
    x, mask = W.synthetic_batch(2, 96, seed=5)
    xg, mg = x.to(dev), mask.to(dev)
    res = []
    for defer, arena in (("0", "0"), ("1", "1"), ("2", "1")):
        monkeypatch.setenv("PN2_DEFER_WGRAD", defer)
        monkeypatch.setenv("PN2_STEP_ARENA", arena)
        tr = Trainer(_fixture_model(fp32=fp32))
        for _ in range(3):          # step 1 torch allocator, step 2 builds the tables on arena addresses, step 3 replays them
            loss = tr.forward_backward(xg, mg)
        torch.cuda.synchronize()
        res.append((loss.clone(), tr.gflat.clone()))
        if defer == "2":
            assert tr.arena.buf is not None and tr.arena.off > 0 and len(tr.grad_queue.cache) >= 1
    for other in res[1:]:
        assert torch.equal(res[0][0], other[0]) and torch.equal(res[0][1], other[1])


@pytest.mark.parametrize("fp32", [False, True, "fp32fast"])
@pytest.mark.parametrize("size", [96, 224])
def test_lockstep_launches_match_plain_launches(fp32, size, monkeypatch):
    """Engine.lockstep (pn2/lockstep.py): the three RFB modules and their branch tails, and the three parallel 3x3 convs of every Res2Net stage
    block, advance position by position on table-driven launches (pn2_conv_gemm_multi, pn2_bn_finalize_multi, pn2_affine_multi,
    pn2_bn_bwd_finalize_multi, pn2_bn_bwd_apply_multi, pn2_bn_bwd_reduce_multi) - against one launch per chain: loss, every gradient and the
    parameters after three optimizer steps, bit for bit; and the launch count drops."""
    from pn2 import engine, capi, core
    from pn2.trainer import Trainer
    from oracle import weights as W
    x, mask = W.synthetic_batch(2, size, seed=6)
    xg, mg = x.to(dev), mask.to(dev)
    res = []
    for on in (False, True):
        monkeypatch.setattr(core, "LOCKSTEP", on)
        tr = Trainer(_fixture_model(fp32=fp32))
        for _ in range(3):          # step 1 torch allocator (no lock step), step 2 builds the tables on arena addresses, step 3 replays them
            loss = tr.step(xg, mg)
        counts = {}
        real = {n: getattr(capi.call, n) for n in ("pn2_conv_gemm", "pn2_conv_gemm_ep", "pn2_conv_gemm_multi", "pn2_bn_finalize", "pn2_bn_finalize_multi")}
        for n, f in real.items():
            monkeypatch.setattr(capi.call, n, lambda *a, _f=f, _n=n: (counts.__setitem__(_n, counts.get(_n, 0) + 1), _f(*a))[1], raising=False)
        loss = tr.forward_backward(xg, mg)
        for n in real:
            monkeypatch.setattr(capi.call, n, real[n], raising=False)
        torch.cuda.synchronize()
        res.append((loss.clone(), tr.gflat.clone(), tr.flat.clone(), counts))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    plain, ls = res[0][3], res[1][3]
    print("launch counts plain", plain, "lock step", ls)
    assert plain.get("pn2_conv_gemm_multi", 0) == 0 and ls["pn2_conv_gemm_multi"] >= 12
    assert ls.get("pn2_conv_gemm", 0) + ls.get("pn2_conv_gemm_ep", 0) + ls["pn2_conv_gemm_multi"] <= plain["pn2_conv_gemm"] + plain["pn2_conv_gemm_ep"] - 50
    assert ls["pn2_bn_finalize_multi"] >= 8 and ls.get("pn2_bn_finalize", 0) + ls["pn2_bn_finalize_multi"] <= plain["pn2_bn_finalize"] - 30


def test_fused_dsra_tail_matches_unfused_path(monkeypatch):
    """pn2_dsra_tail_fwd/_bwd (up-sampling + structure loss + adjoint in two kernels) against the op-by-op path
    (pn2_bilinear_fwd -> pn2_structure_loss_fwd/_bwd -> pn2_bilinear_bwd), fp32 compute, same weights and batch."""
    from pn2.trainer import Trainer
    from oracle import weights as W
    x, mask = W.synthetic_batch(3, 96, seed=8)
    xg, mg = x.to(dev), mask.to(dev)
    res = []
    for fused in ("0", "1"):
        monkeypatch.setenv("PN2_FUSED_TAIL", fused)
        tr = Trainer(_fixture_model(fp32=True))
        loss = tr.forward_backward(xg, mg)
        torch.cuda.synchronize()
        res.append((loss.clone(), tr.last_outs.clone(), tr.gflat.clone()))
    (l0, o0, g0), (l1, o1, g1) = res
    assert relmax(l1, l0) < 2e-6
    assert relmax(o1, o0) < 1e-6
    assert rell2(g1, g0) < 2e-5 and relmax(g1, g0) < 2e-4


TAIL_GEOMS = [  # N, S, align_corners: the three training scales of a 96-pixel fixture, the 1.25x headline scale with align_corners, ragged last band
    (3, 96, 0), (2, 64, 1), (2, 128, 0), (2, 448, 1), (1, 352, 0), (2, 100, 0),
    (1, 640, 0),        # OW > 512: not served by the one-pass kernel
    (2, 256, 0), (2, 448, 0), (3, 352, 0),        # the 0.75x / 1.25x / 1x training scales: 4 / 2 / 2 row lanes, several images per finishing block
]


@pytest.mark.parametrize("cfg", TAIL_GEOMS)
def test_dsra_tail_band_kernels_vs_oracle_and_row_kernels(cfg, monkeypatch):
    """pn2_dsra_tail_fwd/_bwd called through the C ABI on random low-res logits: band kernels (default) and row kernels (PN2_TAIL_BAND=0) against
    the oracle's structure_loss (MyTrain_med.py:19-38) on F.interpolate'd maps in float64 with autograd for the low-res gradients; gradients
    accumulate into pre-filled buffers where `accumulate` is set.  OH = 100 leaves a 4-row last band."""
    import ctypes as C
    from pn2 import capi
    from pn2.capi import call
    from oracle import pranet_oracle as O
    N, S, ac = cfg
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(100 + S)
    sizes = [max(S // 8, 1), max(S // 16, 1), max(S // 32, 1), max(S // 8, 1)]
    src_cpu = [(torch.randn(N, h, h, generator=g) * 2) for h in sizes + sizes]
    mask_cpu = (torch.rand(N, 1, S, S, generator=g) < 0.3).float()
    mask_cpu[:, :, S // 4: S // 2, S // 3: 2 * S // 3] = 1.0
    # ---- oracle (float64, autograd)
    leaves = [t.double().requires_grad_(True) for t in src_cpu]
    ups = [F.interpolate(t[:, None], size=(S, S), mode="bilinear", align_corners=bool(ac)) for t in leaves]
    ref_losses = [O.structure_loss(ups[j], ups[4 + j], mask_cpu.double(), 1 - mask_cpu.double()) for j in range(4)]
    sum(ref_losses).backward()
    ref_grads = [t.grad.float() for t in leaves]
    # the maps themselves are held to the reference's own fp32 index math (float64 source coordinates differ by ~55 * 2^-24 at 448 px, align_corners)
    ups32 = [F.interpolate(t[:, None], size=(S, S), mode="bilinear", align_corners=bool(ac)).reshape(N, S, S) for t in src_cpu]
    res = {}
    pow2 = ac == 0 and S % 32 == 0 and S <= 512 and S // 32 >= 1 and all(S // h in (8, 16, 32) for h in sizes)      # what the one-pass kernel serves
    # the one-pass entry with the fixed-point image-sum accumulators (default in the trainer: two launches) / without (three launches) / band kernels / row kernels
    for band in ("Fi", "F", "1", "0"):
        monkeypatch.setenv("PN2_TAIL_BAND", "2" if band[0] == "F" else band)
        srcs = [t.to(dev) for t in src_cpu]
        base = [torch.randn_like(t) * float(ref_grads[j].abs().max()) for j, t in enumerate(srcs)]      # pre-existing gradient of the sinks that accumulate
        dsrcs = [base[j].clone() if j % 3 == 0 else torch.empty_like(t) for j, t in enumerate(srcs)]
        mask = mask_cpu.reshape(N, S, S).to(dev).contiguous()
        weit = torch.empty_like(mask)
        isum = torch.full((4 * N * 10,), 7, dtype=torch.int64, device=dev) if band == "Fi" else None          # (pn2_loss_weights_clear zeroes it)
        if isum is not None:
            call.pn2_loss_weights_clear(P(mask), P(weit), N, S, S, 31, P(isum), isum.numel(), st)
        else:
            call.pn2_loss_weights(P(mask), P(weit), N, S, S, 31, st)
        d = capi.TailDesc()
        d.N, d.OH, d.OW, d.P, d.align_corners = N, S, S, 4, ac
        for j, (s_, ds) in enumerate(zip(srcs, dsrcs)):
            m, h = d.maps[j], s_.shape[1]
            m.src, m.dsrc, m.h, m.w = s_.data_ptr(), ds.data_ptr(), h, h
            m.rh = m.rw = ((h - 1) / (S - 1) if S > 1 else 0.0) if ac else h / S
            m.accumulate = 1 if j % 3 == 0 else 0
        nb = call.pn2_dsra_tail_blocks(S)
        lat = torch.empty(8, N, S, S, device=dev)
        partial = torch.empty(4, N, nb, 5, device=dev)
        sums, wsum, loss = torch.empty(4, N, 4, device=dev), torch.empty(N, device=dev), torch.empty(5, device=dev)
        fused = int(call.pn2_dsra_tail_fused_ok(C.byref(d)))
        assert fused == (1 if band[0] == "F" and pow2 else 0), (band, fused, pow2)
        if band[0] == "F":
            if not fused:
                continue
            need = int(call.pn2_dsra_tail_fused_scratch(C.byref(d)))
            scratch, per = torch.empty(need, device=dev), torch.empty(4, N, device=dev)
            call.pn2_dsra_tail_fwd_bwd(C.byref(d), P(lat), P(mask), P(weit), P(partial), P(sums), P(wsum), P(per), P(loss), 1.0, P(scratch), need, P(isum), st)
        else:
            need = int(call.pn2_dsra_tail_scratch(C.byref(d)))
            assert (need > 0) == (band == "1")
            scratch = torch.empty(max(need, 1), device=dev)
            call.pn2_dsra_tail_fwd(C.byref(d), P(lat), P(mask), P(weit), P(partial), P(sums), P(wsum), P(loss), st)
            call.pn2_dsra_tail_bwd(C.byref(d), P(mask), P(weit), P(wsum), P(sums), 1.0, P(scratch) if need else None, need, st)
        torch.cuda.synchronize()
        for j in range(8):
            assert relmax(lat[j], ups32[j]) < 2e-6, (band, j)
        for j in range(4):
            assert abs(float(loss[j]) - float(ref_losses[j].detach())) < 5e-6 * abs(float(ref_losses[j].detach())), (band, j)
        assert abs(float(loss[4]) - float(sum(ref_losses).detach())) < 5e-6 * abs(float(sum(ref_losses).detach()))
        for j in range(8):
            got = dsrcs[j] - base[j] if j % 3 == 0 else dsrcs[j]
            assert relmax(got, ref_grads[j]) < 2e-4 and rell2(got, ref_grads[j]) < 2e-5, (band, j, relmax(got, ref_grads[j]), rell2(got, ref_grads[j]))
        res[band] = (lat.clone(), sums.clone(), wsum.clone(), loss.clone(), [t.clone() for j, t in enumerate(dsrcs) if j % 3])          # (the accumulating sinks start from another random base)
    assert relmax(res["1"][0], res["0"][0]) < 1e-6
    if "Fi" in res:     # sums of <= a few thousand fp32 terms are exact in double: the atomically accumulated image sums give the bits of the reduced partial rows
        a, b = res["Fi"], res["F"]
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and all(torch.equal(x, y) for x, y in zip(a[4], b[4]))
    if "F" in res:      # the same maps and per-image sums as the two-call path (another summation order)
        assert relmax(res["F"][0], res["1"][0]) < 1e-6 and relmax(res["F"][1], res["1"][1]) < 2e-6 and relmax(res["F"][2], res["1"][2]) < 2e-6
    # short / missing scratch: the backward falls back to the row kernels instead of failing
    monkeypatch.setenv("PN2_TAIL_BAND", "1")
    call.pn2_dsra_tail_bwd(C.byref(d), P(mask), P(weit), P(wsum), P(sums), 1.0, None, 0, st)
    torch.cuda.synchronize()


def test_pack_weights_multi_matches_single_pack():
    """The one-launch tiled repack (pn2_pack_weights_multi) rewrites every cached panel exactly as pn2_pack_weight builds it."""
    from pn2.trainer import Trainer
    from pn2.engine import PackCache
    from oracle import weights as W
    x, mask = W.synthetic_batch(2, 96, seed=6)
    xg, mg = x.to(dev), mask.to(dev)
    tr = Trainer(_fixture_model(fp32=False))
    tr.forward_backward(xg, mg)                       # panels created by pn2_pack_weight
    first = tr.pack_cache
    with torch.no_grad():
        tr.flat.mul_(1.25).add_(0.01)                 # new master weights
    first.refresh()                                   # multi-job repack in place
    torch.cuda.synchronize()
    tr.pack_cache = PackCache()
    tr.forward_backward(xg, mg)                       # same weights, panels built from scratch by pn2_pack_weight
    torch.cuda.synchronize()
    assert len(first.entries) == len(tr.pack_cache.entries) > 100
    for key, (wp, _) in first.entries.items():
        assert torch.equal(wp, tr.pack_cache.entries[key][0]), key


def test_multiscale_schedule_vs_oracle_and_per_scale_graphs():
    """MyTrain_med.py:55,70-73: every batch is trained at 0.75x, 1x and 1.25x (bilinear, align_corners=True, images and masks).  The trainer
    keeps one warm state (arena, job tables, graphs) per scale; losses are checked against the oracle run on F.interpolate'd inputs."""
    from pn2.trainer import Trainer
    from oracle import weights as W
    from oracle import pranet_oracle as O
    x, mask = W.synthetic_batch(2, 96, seed=21)
    xg, mg = x.to(dev), mask.to(dev)
    sizes = [int(round(96 * r / 32) * 32) for r in (0.75, 1, 1.25)]
    assert sizes == [64, 96, 128]
    tr = Trainer(_fixture_model(fp32=True), lr=1e-4)
    sd = W.make_state_dict(W.manifest_pranet_v2(1), seed=0)
    for S in sizes:
        loss = tr.forward_backward(xg, mg, size=S)
        P = O.clone_sd(sd)
        xr = F.interpolate(x, size=(S, S), mode="bilinear", align_corners=True) if S != 96 else x
        mr = F.interpolate(mask, size=(S, S), mode="bilinear", align_corners=True) if S != 96 else mask
        with torch.no_grad():
            ref = O.total_loss(O.pranet_v2_forward(P, xr, True), mr)
        assert abs(float(loss[-1]) - float(ref)) < 2e-3 * float(ref), (S, float(loss[-1]), float(ref))
        assert tr.last_outs.shape == (8, 2, S, S, 1)
    # bf16: eager multi-scale steps == per-scale captured graphs, bit for bit, over two rounds of the schedule
    res = []
    for graph in (False, True):
        tr = Trainer(_fixture_model(fp32=False), lr=1e-4)
        if graph:
            for S in sizes:
                tr.capture(xg, mg, warmup=2, size=S)          # 2 eager steps per scale, then its graphs
            for _ in range(2):
                for S in sizes:
                    loss = tr.replay(xg, mg, size=S)
        else:
            for S in sizes:
                for _ in range(2):
                    tr.step(xg, mg, size=S)
            for _ in range(2):
                for S in sizes:
                    loss = tr.step(xg, mg, size=S)
        torch.cuda.synchronize()
        res.append((loss.clone(), tr.flat.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_full_size_properties_bs32_352_bf16():
    """BASELINE config 2 shape: size-independent properties instead of an oracle run (which would take minutes on the CPU)."""
    from pn2.trainer import Trainer
    from oracle import weights as W
    x, mask = W.synthetic_batch(32, 352, seed=3)
    xg, mg = x.to(dev), mask.to(dev)
    model = _fixture_model(fp32=False)
    tr = Trainer(model)
    l1 = tr.forward_backward(xg, mg).clone(); g1 = tr.gflat.clone(); o1 = tr.last_outs.clone()
    l2 = tr.forward_backward(xg, mg).clone(); g2 = tr.gflat.clone()
    assert torch.isfinite(l1).all() and torch.isfinite(g1).all()
    assert torch.equal(l1, l2) and torch.equal(g1, g2), "kernels must be deterministic (no atomics on the data path)"
    assert o1.shape == (8, 32, 352, 352, 1)
    # batch-permutation equivariance: BN statistics and the batch-mean loss do not depend on image order
    perm = torch.randperm(32, device=dev)
    l3 = tr.forward_backward(xg[perm], mg[perm])
    assert abs(float(l3[-1]) - float(l1[-1])) < 2e-2 * abs(float(l1[-1]))
    # per-image loss sums: total == sum of the four pair losses
    assert abs(float(l1[:4].sum()) - float(l1[4])) < 1e-5 * abs(float(l1[4]))


def test_inference_predictor_graph_matches_module_eval():
    """pn2.infer.Predictor (eval forward + MyTest_med.py:104-111 tail replayed from one hipGraph) against the nn.Module surface in eval mode
    + pn2.evaltail.test_postprocess: same maps, same uint8 prediction, for two different images through the same captured graph."""
    import time
    from pn2.infer import Predictor
    from pn2.evaltail import test_postprocess
    model = _fixture_model(fp32=False).eval()
    pred = Predictor(model)
    g = torch.Generator(device="cpu").manual_seed(4)
    for k in range(2):
        x = torch.randn(1, 3, 96, 96, generator=g).to(dev)
        with torch.no_grad():
            ref = model(x)
        outs = pred(x)
        assert len(outs) == len(ref)
        for a, b in zip(outs, ref):
            assert torch.equal(a, b)
        u8 = pred.postprocess(x, (123, 77))
        assert torch.equal(u8, test_postprocess(ref, (123, 77)))
    x = torch.randn(1, 3, 352, 352, generator=g).to(dev)
    pred.postprocess(x, (500, 574)); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        pred.postprocess(x, (500, 574))
    torch.cuda.synchronize()
    print(f"\\ninference 1x3x352x352 + tail (hipGraph replay): {(time.perf_counter() - t0) / 20 * 1e3:.2f} ms/image")


def test_untuned_module_eval_returns_the_tuned_predictors_bits(monkeypatch):
    """The intra-workgroup split-K conv kernels sum a tile's K loop in another fp32 order than the plain kernels, so which shapes take them is a rule of the
    shape - and the rule has to hold without the tuner too.  PN2_AUTOTUNE=0 (the nn.Module surface then runs the library heuristics; this is the state an
    earlier test of the suite once leaked into the process) against the Predictor, which always runs tuned tiles: the same bits."""
    from pn2.infer import Predictor
    model = _fixture_model(fp32=False).eval()
    pred = Predictor(model)
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randn(2, 3, 96, 96, generator=g).to(dev)
    monkeypatch.setenv("PN2_AUTOTUNE", "0")
    with torch.no_grad():
        untuned = model(x)
    monkeypatch.setenv("PN2_AUTOTUNE", "1")
    with torch.no_grad():
        tuned = model(x)
    outs = pred(x)
    for a, b, c in zip(outs, untuned, tuned):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_predictor_graphs_survive_a_growing_job_table():
    """a captured inference graph bakes in the device job tables of PackCache / BnFoldCache.  A later input shape that takes another kernel
    path registers new jobs (bs >= 34 at 352^2: the ra4 5x5 convs leave the split-K path, M = 121 * bs > 4096, and add BatchNorm fold entries), which replaces
    the tables.  The replaced tables must stay allocated: the first graph still launches them.  Replay the first shape after the second was captured (with
    allocator churn in between, so a freed table would have been reused) and require the bit-identical maps."""
    from pn2.infer import Predictor
    model = _fixture_model(fp32=False).eval()
    pred = Predictor(model)
    g = torch.Generator(device="cpu").manual_seed(11)
    xa = torch.randn(2, 3, 352, 352, generator=g).to(dev)
    xb = torch.randn(34, 3, 352, 352, generator=g).to(dev)
    first = [o.clone() for o in pred(xa)]
    v0 = (pred.pack_cache.version, pred.bn_fold.version)
    pred(xb)
    grew = (pred.pack_cache.version, pred.bn_fold.version) != v0
    junk = [torch.full((1 << 12,), 0xFF, dtype=torch.uint8, device=dev) for _ in range(256)]      # lands in any small block the allocator got back
    torch.cuda.synchronize()
    again = pred(xa)
    torch.cuda.synchronize()
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    assert grew, "the second shape was meant to register new jobs (otherwise this test does not exercise the retired tables)"
    assert len(pred.pack_cache.retired) + len(pred.bn_fold.retired) >= 1
    del junk


@pytest.mark.parametrize("fp32", [False, True, "fp32fast"])
def test_stem_bn_relu_maxpool_as_one_op(fp32, monkeypatch):
    """conv_bn_act(pool=True): the stem's bn1 -> ReLU -> MaxPool2d(3, 2, 1) (Res2Net_v1b.py:137-139) without the full-resolution BatchNorm output.  Forward
    (pn2_bn_relu_maxpool_fwd): pooled activation and argmax bytes straight from the raw conv output - every value formed as the separate normalise and pool passes form
    it, so with the generic backward (pool-backward launch + BatchNorm passes) a training step agrees BIT FOR BIT with the three separate ops.  Quad backward
    (pn2_pool_bn_bwd_reduce / _apply, the default): no full-resolution gradient tensor either; each pixel's gradient is the same rounded sum, the BatchNorm sums are taken
    in another order - loss and maps identical, gradients equal up to that fp32 order (bf16: plus the roundings of dz that flip with the last bit of the coefficients)."""
    from pn2 import core
    from pn2.trainer import Trainer
    from oracle import weights as W
    for size in (96, 224):          # 48 -> 24 and 112 -> 56 stem maps
        x, mask = W.synthetic_batch(2, size, seed=9)
        xg, mg = x.to(dev), mask.to(dev)
        res = {}
        for name, fuse, quad in (("sep", False, False), ("fwd", True, False), ("quad", True, True)):
            monkeypatch.setattr(core, "POOL_FUSE", fuse)
            monkeypatch.setattr(core, "POOL_BWD_QUAD", quad)
            tr = Trainer(_fixture_model(fp32=fp32))
            loss = tr.forward_backward(xg, mg)
            torch.cuda.synchronize()
            res[name] = (loss.clone(), tr.gflat.clone(), tr.last_outs.clone())
        for name in ("fwd", "quad"):
            assert torch.equal(res["sep"][0], res[name][0]) and torch.equal(res["sep"][2], res[name][2]), name
        assert torch.equal(res["sep"][1], res["fwd"][1]), float((res["sep"][1] - res["fwd"][1]).abs().max())
        rel = float((res["sep"][1] - res["quad"][1]).norm() / res["sep"][1].norm())
        print(f"\nstem pool quad backward vs separate ops, {fp32 if isinstance(fp32, str) else ('fp32' if fp32 else 'bf16')} {size}^2: gradient rel-L2 {rel:.2e}")
        # bf16: a handful of dz roundings flip with the last bit of the stem's coefficients and the net amplifies them: 5e-8 ... 8e-5 observed over runs of the same
        # code (which flips occur depends on the tiles / pixel splits the tuner timed fastest in that process); the bf16 gradient noise itself is ~1e-2
        assert rel <= (2e-7 if fp32 else 1e-3), rel
