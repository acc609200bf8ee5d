"""GPU tests of EMCADNet(dual, K=9) with the PVTv2-B0 encoder (head_dim 32 in every stage): the head_dim-32 attention kernels through the C ABI
against float64 torch, the ops of the b0 path at their own widths, the backbone and the whole model against the oracle / the imported reference
(tests/golden/emcad_b0_128.npz), and the bf16 Trainer at full size."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
os.environ.setdefault("PN2_NO_PRETRAINED", "1")
import emcad_b0ref as R  # noqa: E402
from test_gpu_pvt import _run, relmax, rell2  # noqa: E402
from test_gpu_emcad import _check, _randomize  # noqa: E402

dev = "cuda"


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()
    yield
    pn2.set_compute_dtype("bf16")


# ------------------------------------------------------------------------------------------ attention at head_dim 32 through the C ABI
P_ = lambda t: C.c_void_p(t.data_ptr())
# (heads, Nq, Nkv): every 64-key bucket, the 129..192 -> 256-key instantiation, partial last query / key tiles
ATTN_CASES = [(1, 1, 1), (2, 63, 7), (5, 130, 49), (8, 3136, 64), (1, 130, 65), (2, 3136, 121), (8, 63, 129), (5, 1, 200), (1, 3136, 256),
              (8, 130, 256), (2, 1, 256), (5, 3136, 7)]
HD = 32


def _attn(dtn, heads, Nq, Nkv, pad_q, pad_kv, B=2):
    from pn2 import capi, F32, BF16
    dt, tdt = (F32, torch.float32) if dtn == "fp32" else (BF16, torch.bfloat16)
    Cc = heads * HD
    ldq, ldkv = Cc + pad_q, 2 * Cc + pad_kv
    g = torch.Generator().manual_seed(heads * 1000 + Nq + Nkv)
    q, kv, do = torch.randn(B, Nq, Cc, generator=g), torch.randn(B, Nkv, 2 * Cc, generator=g), torch.randn(B, Nq, Cc, generator=g)

    def view(t, ld):                                    # channel slice of a wider buffer; the columns past the slice hold NaN
        buf = torch.full((t.shape[0], t.shape[1], ld), float("nan"), dtype=tdt, device=dev)
        if t is not None:
            buf[..., :t.shape[2]] = t.to(tdt)
        return buf
    qb, kvb, dob = view(q, ldq), view(kv, ldkv), view(do, ldq)
    ob, dqb, dkvb = view(torch.zeros(B, Nq, 0), ldq), view(torch.zeros(B, Nq, 0), ldq), view(torch.zeros(B, Nkv, 0), ldkv)
    lse = torch.empty(B, heads, Nq, device=dev); delta = torch.empty(B, heads, Nq, device=dev)
    nb = capi.call.pn2_attn_bwd_blocks(dt, B, heads, Nq)
    part = torch.empty(B, heads, nb, 2, (Nkv + 63) // 64 * 64, HD, device=dev)        # the head_dim-32 partial layout of pn2.h
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sc = HD ** -0.5
    capi.call.pn2_attn_fwd(dt, P_(qb), ldq, P_(kvb), ldkv, P_(ob), ldq, P_(lse), B, Nq, Nkv, heads, HD, sc, st)
    capi.call.pn2_attn_bwd(dt, P_(qb), ldq, P_(kvb), ldkv, P_(ob), ldq, P_(dob), ldq, P_(lse), P_(dqb), ldq, P_(dkvb), ldkv, P_(part), P_(delta),
                           B, Nq, Nkv, heads, HD, sc, st)
    torch.cuda.synchronize()
    cast = (lambda t: t.bfloat16().double()) if dtn == "bf16" else (lambda t: t.double())
    q64, kv64 = cast(q).requires_grad_(True), cast(kv).requires_grad_(True)
    qq = q64.reshape(B, Nq, heads, HD).transpose(1, 2)
    kk = kv64.reshape(B, Nkv, 2, heads, HD).permute(2, 0, 3, 1, 4)
    r = ((qq @ kk[0].transpose(-2, -1)) * sc).softmax(-1) @ kk[1]
    r = r.transpose(1, 2).reshape(B, Nq, Cc)
    r.backward(cast(do))
    err, tol = (relmax, 5e-5) if dtn == "fp32" else (rell2, 3e-2)
    assert err(ob[..., :Cc].float(), r) < tol, "forward"
    assert err(dqb[..., :Cc].float(), q64.grad) < tol, "dq"
    assert err(dkvb[..., :2 * Cc].float(), kv64.grad) < tol, "dkv"
    for t, n in ((ob, Cc), (dqb, Cc), (dkvb, 2 * Cc)):
        assert bool(torch.isnan(t[..., n:].float()).all()), "wrote past the row"


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ATTN_CASES)
def test_attention_hd32_c_abi(dtn, case):
    heads, Nq, Nkv = case
    _attn(dtn, heads, Nq, Nkv, 0, 0)                    # ld = heads * 32 (the MFMA kernels for bf16)
    _attn(dtn, heads, Nq, Nkv, 16, 8)                   # channel slice of a wider buffer
    if dtn == "bf16":
        _attn(dtn, heads, Nq, Nkv, 4, 12)               # ld not a multiple of 8: the scalar kernels


def test_attention_other_head_dims_refused():
    from pn2 import capi, BF16, F32
    lib = capi.load()
    buf = torch.zeros(1 << 16, device=dev)
    p, st = P_(buf), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for dt in (F32, BF16):
        for hd in (16, 48, 128):
            assert lib.pn2_attn_fwd(dt, p, 2 * hd, p, 4 * hd, p, 2 * hd, p, 1, 16, 16, 2, hd, 0.1, st) == -2, hd
            assert lib.pn2_attn_bwd(dt, p, 2 * hd, p, 4 * hd, p, 2 * hd, p, 2 * hd, p, p, 2 * hd, p, 4 * hd, p, p, 1, 16, 16, 2, hd, 0.1, st) == -2, hd
        for nkv in (0, 257):
            assert lib.pn2_attn_fwd(dt, p, 64, p, 128, p, 64, p, 1, 16, nkv, 2, 32, 0.1, st) == -2, nkv


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
def test_attention_hd32_engine(dtn):
    """Engine.attention (pn2/ops_encoder.py) at the b0 stage geometries: hd = C / heads = 32, the partial allocated for hd 32."""
    from pn2 import F32, BF16
    from pn2.engine import Engine
    from pn2.graph import _seed_grad
    dt = F32 if dtn == "fp32" else BF16
    err, tol = (relmax, 5e-5) if dt == F32 else (rell2, 3e-2)
    for heads, (qh, qw), (kh, kw) in ((1, (16, 16), (2, 2)), (2, (8, 8), (2, 2)), (5, (4, 4), (2, 2)), (8, (2, 2), (2, 2)), (1, (28, 28), (11, 11))):
        torch.manual_seed(heads)
        B, Cc = 2, heads * HD
        q = torch.randn(B, Cc, qh, qw, device=dev); kv = torch.randn(B, 2 * Cc, kh, kw, device=dev)
        eng = Engine(dt, True, need_grad=True)
        qa, kva = eng.from_nchw(q, True), eng.from_nchw(kv, True)
        o = eng.attention(qa, kva, heads)
        out = eng.to_nchw(o).clone()
        go = torch.randn_like(out)
        _seed_grad(o, go); eng.backward()
        cast = (lambda t: t.bfloat16().float()) if dt == BF16 else (lambda t: t)
        q64 = cast(q).double().cpu().requires_grad_(True); kv64 = cast(kv).double().cpu().requires_grad_(True)
        Nq, Nkv = qh * qw, kh * kw
        qq = q64.flatten(2).transpose(1, 2).reshape(B, Nq, heads, HD).permute(0, 2, 1, 3)
        kk = kv64.flatten(2).transpose(1, 2).reshape(B, Nkv, 2, heads, HD).permute(2, 0, 3, 1, 4)
        r = (((qq @ kk[0].transpose(-2, -1)) * HD ** -0.5).softmax(dim=-1) @ kk[1]).transpose(1, 2).reshape(B, Nq, Cc).transpose(1, 2).reshape(B, Cc, qh, qw)
        r.backward(go.double().cpu())
        assert err(out, r) < tol
        assert err(qa.grad.float().permute(0, 3, 1, 2), q64.grad) < tol
        assert err(kva.grad.float().permute(0, 3, 1, 2), kv64.grad) < tol


# ------------------------------------------------------------------------------------------ the other ops of the b0 path at their widths
@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
@pytest.mark.parametrize("C_", [32, 160, 256])
def test_layernorm_b0_widths(dtn, C_):
    torch.manual_seed(C_)
    ln = nn.LayerNorm(C_, eps=1e-6).to(dev)
    ln.weight.data.uniform_(0.5, 1.5); ln.bias.data.normal_(0, 0.2)
    x = torch.randn(3, C_, 7, 5, device=dev) * 2 + 0.3
    _run(dtn, lambda e, a: e.layernorm(a, ln),
         lambda t, g, b: F.layer_norm(t.permute(0, 2, 3, 1), (C_,), g, b, 1e-6).permute(0, 3, 1, 2), x, [ln.weight, ln.bias])


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
def test_linear_and_convs_b0_widths(dtn):
    torch.manual_seed(5)
    for cin, cout in ((32, 32), (32, 64), (32, 256), (256, 32)):
        lin = nn.Linear(cin, cout).to(dev)
        x = torch.randn(2, cin, 6, 9, device=dev)
        _run(dtn, lambda e, a: e.linear(a, lin), lambda t, w, b: F.linear(t.permute(0, 2, 3, 1), w, b).permute(0, 3, 1, 2), x, [lin.weight, lin.bias])
    for (cin, cout, k, s, p, H) in ((32, 64, 3, 2, 1, 13), (32, 32, 8, 8, 0, 24)):       # patch_embed2, stage-1 spatial reduction
        conv = nn.Conv2d(cin, cout, k, s, p).to(dev)
        conv.bias.data.normal_(0, 0.2)
        xx = torch.randn(2, cin, H, H, device=dev)
        _run(dtn, lambda e, a: e.conv_bias(a, conv), lambda t, w, b: F.conv2d(t, w, b, s, p), xx, [conv.weight, conv.bias])
    conv = nn.Conv2d(256, 256, 3, 1, 1, groups=256).to(dev)                            # stage-4 Mix-FFN
    conv.weight.data.normal_(0, 0.4); conv.bias.data.normal_(0, 0.3)
    _run(dtn, lambda e, a: e.dwconv_gelu(a, conv), lambda t, w, b: F.gelu(F.conv2d(t, w, b, 1, 1, groups=256)), torch.randn(2, 256, 5, 6, device=dev),
         [conv.weight, conv.bias])


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
def test_decoder_blocks_b0_widths(dtn):
    from lib.decoders import LGAG, CAB, MSCB, EUCB
    from oracle import emcad_oracle as E
    from oracle.pranet_oracle import Ctx
    l = _randomize(LGAG(32, 32, 16, kernel_size=3, groups=16), 3)
    g, x = torch.randn(2, 32, 7, 6, device=dev), torch.randn(2, 32, 7, 6, device=dev)      # the map size of test_gpu_emcad.py::test_gates_lgag_cab_sab: the bf16
    # bound on the analytically-zero psi bias gradient (a sum over the pixels of rounded terms) is set for it
    _check(dtn, l, lambda e, a, b: l._build(e, a, b), lambda P, a, b: E.lgag(P, "", a, b, Ctx(True)), [g, x])
    c = _randomize(CAB(32), 4)                                                          # 2 hidden channels
    xc = torch.randn(3, 32, 6, 5, device=dev)
    _check(dtn, c, lambda e, a: c._build_gated(e, a), lambda P, t: E.cab(P, "", t) * t, [xc])
    m = _randomize(MSCB(32, 32, 1, kernel_sizes=[1, 3, 5], expansion_factor=2, activation="relu6"), 1)
    _check(dtn, m, lambda e, a: m._build(e, a), lambda P, t: E.mscb(P, "", t, Ctx(True)), [torch.randn(2, 32, 11, 9, device=dev) * 1.5])
    u = _randomize(EUCB(64, 32), 2)
    _check(dtn, u, lambda e, a: u._build(e, a), lambda P, t: E.eucb(P, "", t, Ctx(True)), [torch.randn(2, 64, 5, 6, device=dev)])


def test_emcad_dual_decoder_b0_vs_oracle_fp32():
    """The whole decoder at the b0 channels [256, 160, 64, 32] against the oracle in float64, bounds of test_emcad_dual_decoder_vs_oracle_fp32."""
    from pn2 import F32
    from pn2.engine import Engine
    from pn2.graph import _seed_grad
    from lib.decoders import EMCAD_dual
    from oracle import emcad_oracle as E
    from oracle.pranet_oracle import Ctx
    dec = _randomize(EMCAD_dual(channels=list(R.CHANNELS), kernel_sizes=[1, 3, 5], expansion_factor=2, activation="relu6", num_class=9), 7)
    torch.manual_seed(8)
    feats = [torch.randn(3, c, s, s, device=dev) for c, s in zip(R.CHANNELS, (6, 12, 24, 48))]
    eng = Engine(F32, True, need_grad=True)
    acts = [eng.from_nchw(f, requires_grad=True) for f in feats]
    outs = dec._build(eng, acts[0], acts[1:])
    o_t = [eng.to_nchw(o).clone() for o in outs]
    torch.manual_seed(99)
    gys = [torch.randn_like(o) for o in o_t]
    for o, g in zip(outs, gys):
        _seed_grad(o, g)
    eng.backward()

    def oracle(dtype):
        P = {k: (v.detach().to(dtype).cpu().clone() if v.dtype.is_floating_point else v.detach().cpu().clone()) for k, v in dec.state_dict().items()}
        for k, v in P.items():
            if v.dtype.is_floating_point and not k.endswith(("running_mean", "running_var")):
                v.requires_grad_(True)
        fx = [f.to(dtype).cpu().requires_grad_(True) for f in feats]
        ref = E.emcad_dual(P, "", fx[0], fx[1:], Ctx(True))
        sum((r * g.to(dtype).cpu()).sum() for r, g in zip(ref, gys)).backward()
        return P, fx, ref
    P, f64, ref = oracle(torch.float64)
    P32, f32, _ = oracle(torch.float32)
    for i, (o, r) in enumerate(zip(o_t, ref)):
        assert relmax(o, r) < 2e-4, i
    for a, f, fr, fr32 in zip(acts, feats, f64, f32):
        assert rell2(a.grad[..., :f.shape[1]].permute(0, 3, 1, 2), fr.grad) < max(1e-2, 8 * rell2(fr32.grad, fr.grad))
    for k, p in dec.named_parameters():
        g = eng.pgrads.get(p)
        if float(P[k].grad.abs().max()) < 1e-6:
            assert float(g.abs().max()) < 2e-3, k
        else:
            floor = 2.5e-2 if p.numel() == 1 else 1e-2
            assert rell2(g, P[k].grad) < max(floor, 8 * rell2(P32[k].grad, P[k].grad)), k


# ------------------------------------------------------------------------------------------ backbone and whole model
def _model(mode="fp32"):
    import pn2
    from lib.networks import EMCADNet
    pn2.set_compute_dtype(mode)
    m = EMCADNet(num_classes=9, kernel_sizes=[1, 3, 5], expansion_factor=2, dw_parallel=True, add=True, lgag_ks=3, activation="relu6", encoder="pvt_v2_b0",
                 pretrain=False, dual=True)
    m.load_state_dict(R.state_dict(seed=5), strict=True)
    m.backbone.reset_drop_path(0.0)
    return m.to(dev).train()


def test_pvt_b0_backbone_features_vs_oracle():
    from oracle.pranet_oracle import pvt_features
    model = _model("fp32")
    g = torch.Generator().manual_seed(4321)
    x = torch.randn(2, 3, 128, 128, generator=g)
    with torch.no_grad():
        feats = model.backbone(x.to(dev))
    sd = R.state_dict(seed=5)
    ref = {dt: [f.detach() for f in pvt_features({k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}, "backbone.", x.to(dt), R.PVT_B0)]
           for dt in (torch.float32, torch.float64)}
    for i, f in enumerate(feats):
        own = float((ref[torch.float32][i].double() - ref[torch.float64][i]).abs().max())
        assert tuple(f.shape) == tuple(ref[torch.float64][i].shape), i
        assert float((f.double().cpu() - ref[torch.float64][i]).abs().max()) <= max(1e-4, 3 * own), i


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp32fast"])
def test_emcadnet_b0_forward_backward_vs_reference(mode):
    from pn2.loss import mutation_loss
    z, x, label, bg = R.fixture()
    sub = int(z["sub"])
    model = _model(mode)
    outs = model(x.to(dev), mode="train")
    loss = mutation_loss(outs, label.to(dev), bg.to(dev))
    loss.backward()
    names = dict(model.named_parameters())
    # gradient probes: fp32 within 3x the reference's own fp32 distance to float64.  fp32fast (PN2_F32F: contractions with fewer correctly
    # rounded steps) meets the fp32 gates on the maps and the loss; its gradient probes get a relative floor of 5e-3 on top of the 3x band
    # (measured: norm of backbone.block2.1.attn.kv.weight 1.7e-3 off, the head of backbone.block1.0.attn.kv.weight 5.0e-3 against the
    # reference fp32 run's own 4.0e-3)
    band, rel = 3, (5e-3 if mode == "fp32fast" else 1e-4)
    if mode != "bf16":
        for i, o in enumerate(outs):
            ref64 = torch.from_numpy(z[f"f64.out{i}"]).double()
            assert float((o.detach()[:, :, ::sub, ::sub].double().cpu() - ref64).abs().max()) <= max(1e-4, 3 * float(z[f"own.out{i}"])), i
        assert abs(float(loss.detach()) - float(z["f64.loss"])) < max(1e-4, 3 * abs(float(z["loss"]) - float(z["f64.loss"])))
        for k in z.files:
            if k.startswith("f64.grawnorm."):
                name = k[len("f64.grawnorm."):]
                g = names[name].grad
                r64, r32 = float(z[k]), float(z["grawnorm." + name])
                assert abs(float(g.norm()) - r64) <= max(rel * r64, band * abs(r32 - r64)) + 2e-6, name
                h64 = torch.from_numpy(z["f64.graw." + name]).double(); h32 = torch.from_numpy(z["graw." + name]).double()
                ours = g.detach().reshape(-1)[:h64.numel()].double().cpu()
                assert float((ours - h64).norm()) <= max(rel * float(h64.norm()), band * float((h32 - h64).norm())) + 2e-6, name
    else:
        rels = [rell2(o.detach()[:, :, ::sub, ::sub], torch.from_numpy(z[f"f64.out{i}"])) for i, o in enumerate(outs)]
        print("\nEMCADNet-b0 bf16 128x128, rel-L2 of the 8 maps against the reference's float64 run:", " ".join(f"{v:.3f}" for v in rels))
        # sanity band of test_gpu_emcad.py (b2, 64^2: the last map of each head 0.22-0.27): the error grows stage by stage through the decoder's
        # train-mode BatchNorms, measured 0.027 / 0.053 / 0.101 / 0.167 per head here; fp32 and fp32fast above carry the tight gates
        for i, v in enumerate(rels):
            assert v < 0.35, i
        assert abs(float(loss.detach()) - float(z["f64.loss"])) < 5e-2 * float(z["f64.loss"])


@pytest.mark.parametrize("N,S", [(16, 512), (6, 224)])
def test_trainer_b0_full_size_properties_bf16(N, S):
    """bf16 Trainer(loss="mutation", AdamW) on EMCADNet-b0: finite, deterministic, sample-permutation invariant, hipGraph replay == eager."""
    from pn2.trainer import Trainer
    g = torch.Generator(device="cpu").manual_seed(77)
    K = 9
    x = torch.randn(N, 1, S, S, generator=g).to(dev)
    lab = torch.randint(0, K, (N, S // 16, S // 16), generator=g).to(dev)
    lab = torch.nn.functional.interpolate(lab[:, None].float(), size=(S, S), mode="nearest")[:, 0].long()
    bg = torch.stack([(lab != k).float() for k in range(K)], 1)

    def trainer():
        m = _model("bf16")
        return Trainer(m, lr=1e-4, clip=None, weight_decay=1e-4, loss="mutation", hot=m.hot_parameters(True))
    tr = trainer()
    l1 = tr.forward_backward(x, (lab, bg)).clone(); g1 = tr.gflat.clone()
    l2 = tr.forward_backward(x, (lab, bg)).clone(); g2 = tr.gflat.clone()
    assert torch.isfinite(l1).all() and torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    perm = torch.randperm(N, device=dev)
    l3 = tr.forward_backward(x[perm], (lab[perm], bg[perm]))
    assert abs(float(l3[0]) - float(l1[0])) < 2e-2 * abs(float(l1[0]))
    ref = trainer()
    for _ in range(3):
        le = ref.step(x, (lab, bg))
    cap = trainer()
    cap.capture(x, (lab, bg), warmup=2)
    lg = cap.replay(x, (lab, bg))
    torch.cuda.synchronize()
    assert torch.equal(le, lg) and torch.equal(ref.flat, cap.flat)
