"""GPU tests of the EMCAD decoder switches: pn2_msdc_combine / pn2_msdc_combine_bwd bit for bit against tests/msdcref.py, the engine ops on top of them, the seven
configurations of tests/golden/emcad_sw_*.npz through the module surface, Trainer capture / replay and VolumePredictor on the configuration with every switch
turned, and the default configuration's launches."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import emcad_swref as S
import msdcref as R

pytestmark = pytest.mark.gpu
os.environ.setdefault("PN2_NO_PRETRAINED", "1")
dev = "cuda"
F32, BF16 = 0, 1
MODES = {"sum": 0, "cat": 1}
CANARY = {F32: 0x7FC00123, BF16: 0x7FC1}


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()
    yield
    pn2.set_compute_dtype("bf16")


# ------------------------------------------------------------------------------------------------ the kernel, bit for bit
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _to_dev(bits, dt):
    """numpy bit patterns (uint32 / uint16) -> device tensor of the storage type"""
    if dt == F32:
        return torch.from_numpy(bits.view(np.float32).copy()).to(dev)
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16).to(dev)


def _bits(t, dt):
    return t.cpu().numpy().view(np.uint32) if dt == F32 else t.cpu().view(torch.int16).numpy().view(np.uint16)


def _value(bits, dt):
    return bits.view(np.float32) if dt == F32 else R.bf16_value(bits)


def _as_bits(v, dt):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32) if dt == F32 else R.bf16_bits(v)


class _Pool:
    """storage-representable random values with -0.0, subnormals and the largest finite value sprinkled in, cut from one array"""

    def __init__(self, dt, seed, n=1 << 21):
        rng = np.random.default_rng(seed)
        v = _as_bits(rng.standard_normal(n).astype(np.float32) * 2.0, dt).copy()
        special = [0x80000000, 0x00000001, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF] if dt == F32 else [0x8000, 0x0001, 0x807F, 0x7F7F, 0xFF7F]
        pos = rng.integers(0, n, size=n // 16)
        v[pos] = np.asarray(special, dtype=v.dtype)[rng.integers(0, len(special), size=pos.size)]
        v[:len(special)] = special                        # every case starts inside the specials
        self.v, self.at = v, 0

    def take(self, M, Cc):
        k = M * Cc
        if self.at + k > self.v.size:
            self.at = 0
        out = self.v[self.at:self.at + k].reshape(M, Cc)
        self.at += max(k // 2, 1)
        return out


def _guarded(M, Cc, dt, fill=None):
    """[M + 2][Cc] device buffer of canary patterns (rows 1..M optionally pre-filled), the view of rows 1..M"""
    b = np.full((M + 2, Cc), CANARY[dt], dtype=np.uint32 if dt == F32 else np.uint16)
    if fill is not None:
        b[1:M + 1] = fill
    t = _to_dev(b, dt)
    return t, t[1:M + 1]


def _canaries_intact(t, dt):
    b = _bits(t, dt)
    return bool((b[0] == CANARY[dt]).all() and (b[-1] == CANARY[dt]).all())


def _shapes(lib, dt, mode):
    """(Cpart, n, groups, M): every part count and shuffle at each width, M around the kernel's own tile"""
    for Cpart in (8, 24, 64, 100 if dt == F32 else 200, 3072):
        for n in (1, 2, 3, 4):
            Cw = n * Cpart if mode != "sum" else Cpart
            p2 = Cw & -Cw                                  # the largest power of two in Cw: Cw / p2 is odd
            for groups in sorted({g for g in (1, 2, Cpart, Cw, p2) if Cw % g == 0}):
                tile = lib.pn2_msdc_combine_tile(dt, Cw, Cw // groups if mode == "bwd" else groups)
                assert tile >= 1
                for M in sorted({m for m in (1, tile - 1, tile + 1, 3 * tile + 5) if m >= 1}):
                    yield Cpart, n, groups, M
    if mode != "sum":
        yield 4096, 4, 4096, 2                             # Cw = 16384, the widest built row (fp32: the whole default LDS, unpadded)
        yield 4096, 4, 4, 3
    else:
        yield 16384, 2, 8192, 2


@pytest.mark.parametrize("mode", ["sum", "cat"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
def test_msdc_combine_matches_numpy_bitwise(dt, mode):
    from pn2 import capi
    lib = capi.load()
    pool = _Pool(dt, 7 + dt)
    null = C.c_void_p(0)
    ncase = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for Cpart, n, groups, M in _shapes(lib, dt, mode):
            parts = [pool.take(M, Cpart) for _ in range(n)]
            want = _as_bits(R.combine([_value(p, dt) for p in parts], groups, mode, bf16=dt == BF16), dt)
            if mode == "cat" or n == 1:                    # a pure move: the patterns themselves, specials included
                moved = np.concatenate(parts, axis=1)[:, R.src_index(want.shape[1], groups)]
                assert np.array_equal(want, moved)
            dparts = [_to_dev(p, dt) for p in parts]
            buf, y = _guarded(M, want.shape[1], dt)
            ps = [C.c_void_p(t.data_ptr()) for t in dparts] + [null] * (4 - n)
            rc = lib.pn2_msdc_combine(dt, MODES[mode], n, ps[0], ps[1], ps[2], ps[3], C.c_void_p(y.data_ptr()), M, Cpart, groups, _stream())
            assert rc == 0, (rc, Cpart, n, groups, M)
            got = _bits(buf, dt)
            assert np.array_equal(got[1:M + 1], want), (Cpart, n, groups, M)
            assert _canaries_intact(buf, dt), (Cpart, n, groups, M)
            ncase += 1
    assert ncase > 200


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
def test_msdc_combine_bwd_matches_numpy_bitwise(dt):
    from pn2 import capi
    lib = capi.load()
    pool = _Pool(dt, 17 + dt)
    null = C.c_void_p(0)
    ncase = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for Cpart, n, groups, M in _shapes(lib, dt, "bwd"):
            Cw = n * Cpart
            dy = pool.take(M, Cw)
            pre = [pool.take(M, Cpart) for _ in range(n)]
            for acc in ([0] * n, [1] * n, [(i + 1) % 2 for i in range(n)]):
                want = R.combine_bwd(_value(dy, dt), n, groups, prefill=[_value(p, dt) for p in pre], accumulate=acc, bf16=dt == BF16)
                bufs = [_guarded(M, Cpart, dt, fill=p) for p in pre]
                ddy = _to_dev(dy, dt)
                ps = [C.c_void_p(v.data_ptr()) for _, v in bufs] + [null] * (4 - n)
                a4 = acc + [0] * (4 - n)
                rc = lib.pn2_msdc_combine_bwd(dt, n, C.c_void_p(ddy.data_ptr()), ps[0], ps[1], ps[2], ps[3], a4[0], a4[1], a4[2], a4[3], M, Cpart, groups, _stream())
                assert rc == 0, (rc, Cpart, n, groups, M)
                for i, (buf, _) in enumerate(bufs):
                    assert np.array_equal(_bits(buf, dt)[1:M + 1], _as_bits(want[i], dt)), (Cpart, n, groups, M, acc, i)
                    assert _canaries_intact(buf, dt), (Cpart, n, groups, M, acc, i)
                if n == 1 and acc[0] == 0:                 # the adjoint of the sum is the sum of one tensor through the inverse shuffle: the same bits
                    buf, y = _guarded(M, Cw, dt)
                    assert lib.pn2_msdc_combine(dt, 0, 1, C.c_void_p(ddy.data_ptr()), null, null, null, C.c_void_p(y.data_ptr()), M, Cw, Cw // groups, _stream()) == 0
                    assert np.array_equal(_bits(buf, dt)[1:M + 1], _as_bits(want[0], dt)) and _canaries_intact(buf, dt)
                ncase += 1
    assert ncase > 600


# ------------------------------------------------------------------------------------------------ the engine ops
def _shuffle(x, groups):
    N, Cc, H, W = x.shape
    return x.view(N, groups, Cc // groups, H, W).transpose(1, 2).contiguous().view(N, Cc, H, W)


@pytest.mark.parametrize("n", [2, 4])
def test_engine_shuffled_ops_with_a_second_consumer_fp32(n):
    """shuffled_cat and shuffled_sum(shared_grad=False) where part 0 also feeds an add (the sequential MSDC): forward and every part's gradient against torch
    autograd in fp32 - moves, and sums of at most two terms per element, so bit for bit."""
    from pn2 import F32 as DT
    from pn2.engine import Engine
    from pn2.graph import _seed_grad
    g = torch.Generator().manual_seed(n)
    Cc, groups = 24, 8
    for op in ("cat", "sum"):
        xs = [torch.randn(2, Cc, 5, 7, generator=g).to(dev) for _ in range(n)]
        eng = Engine(DT, True, need_grad=True)
        acts = [eng.from_nchw(x, True) for x in xs]
        side = eng.add(acts[0], acts[1])
        y = eng.shuffled_cat(acts, groups) if op == "cat" else eng.shuffled_sum(acts, groups, shared_grad=False)
        out, out_side = eng.to_nchw(y).clone(), eng.to_nchw(side).clone()
        gy, gs = torch.randn(out.shape, generator=g).to(dev), torch.randn(out_side.shape, generator=g).to(dev)
        _seed_grad(y, gy); _seed_grad(side, gs)
        eng.backward()
        ts = [x.clone().requires_grad_(True) for x in xs]
        if op == "cat":
            ref = _shuffle(torch.cat(ts, 1), groups)
        else:
            ref = ts[0]
            for t in ts[1:]:
                ref = ref + t
            ref = _shuffle(ref, groups)
        (ts[0] + ts[1]).backward(gs)
        ref.backward(gy)
        assert torch.equal(out, ref.detach())
        for a, t in zip(acts, ts):
            assert torch.equal(a.grad[..., :Cc].permute(0, 3, 1, 2), t.grad), op


def test_default_configuration_keeps_its_launches(monkeypatch):
    """[1,3,5] / parallel / add: the combine step is pn2_gather_sum forward and backward (one each per MSCB), the new entry points are never called, and the three
    branch outputs of an MSCB share ONE gradient tensor."""
    import pn2
    from pn2 import BF16 as DT
    from pn2.capi import call
    from pn2.engine import Engine
    from pn2.graph import _seed_grad
    from lib.networks import EMCADNet
    from pn2.loss import mutation_loss
    counts = {}
    for name in ("pn2_gather_sum", "pn2_msdc_combine", "pn2_msdc_combine_bwd"):
        real = getattr(call, name)
        monkeypatch.setattr(call, name, lambda *a, _r=real, _n=name: (counts.__setitem__(_n, counts.get(_n, 0) + 1), _r(*a))[1], raising=False)
    pn2.set_compute_dtype("bf16")
    m = EMCADNet(num_classes=S.K, activation="relu6", encoder="pvt_v2_b0", pretrain=False, dual=True, **S.DEFAULT)
    m.backbone.reset_drop_path(0.0)
    m = m.to(dev).train()
    _, x, label, bg = S.fixture("cat")
    mutation_loss(m(x.to(dev), mode="train"), label.to(dev), bg.to(dev)).backward()
    torch.cuda.synchronize()
    assert counts == {"pn2_gather_sum": 8}, counts
    eng = Engine(DT, True, need_grad=True)
    parts = [eng.from_nchw(torch.randn(2, 64, 6, 5, device=dev), True) for _ in range(3)]
    y = eng.shuffled_sum(parts, 32)
    _seed_grad(y, torch.randn(2, 64, 6, 5, device=dev))
    eng.backward()
    assert counts == {"pn2_gather_sum": 10}, counts
    assert parts[0].grad.data_ptr() == parts[1].grad.data_ptr() == parts[2].grad.data_ptr()


# ------------------------------------------------------------------------------------------------ whole models
def _model(name, mode):
    import pn2
    pn2.set_compute_dtype(mode)
    return S.build(name).to(dev).train()


def _loss(name, outs, label, bg):
    from pn2.loss import mutation_loss, seg_loss
    return mutation_loss(outs, label, bg) if S.CONFIGS[name][1] else seg_loss(outs, label)


def rell2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", S.NAMES)
def test_switch_models_forward_backward_vs_reference(name, mode):
    """The module surface (eager forward + mutation loss + backward) against the reference's float64 run, with the gates and multipliers of
    test_gpu_pvt_b0.py::test_emcadnet_b0_forward_backward_vs_reference: fp32 within 3 x the reference's own fp32-to-float64 distance (floors 1e-4), bf16 in its
    sanity band."""
    z, x, label, bg = S.fixture(name)
    sub = int(z["sub"])
    model = _model(name, mode)
    outs = model(x.to(dev), mode="train")
    assert len(outs) == (8 if S.CONFIGS[name][1] else 4)
    loss = _loss(name, outs, label.to(dev), bg.to(dev))
    loss.backward()
    names = dict(model.named_parameters())
    band, rel = 3, 1e-4
    if mode != "bf16":
        for i, o in enumerate(outs):
            ref64 = torch.from_numpy(z[f"f64.out{i}"]).double()
            err, own = float((o.detach()[:, :, ::sub, ::sub].double().cpu() - ref64).abs().max()), float(z[f"own.out{i}"])
            print(f"\n{name} map {i}: |ours - f64| {err:.2e}, the reference's own {own:.2e}")
            assert err <= max(1e-4, 3 * own), i
        assert abs(float(loss.detach()) - float(z["f64.loss"])) < max(1e-4, 3 * abs(float(z["loss"]) - float(z["f64.loss"])))
        probes = [k[len("f64.grawnorm."):] for k in z.files if k.startswith("f64.grawnorm.")]
        last = len(S.switches(name)["kernel_sizes"]) - 1
        assert {"decoder.mscb1.0.msdc.dwconvs.0.0.weight", f"decoder.mscb1.0.msdc.dwconvs.{last}.0.weight", "decoder.mscb1.0.pconv2.0.weight", "decoder.lgag1.W_g.0.weight",
                "decoder.lgag1.W_g.0.bias", "decoder.mscb4.0.pconv1.0.weight"} <= set(probes)
        for pname in probes:
            g = names[pname].grad
            r64, r32 = float(z["f64.grawnorm." + pname]), float(z["grawnorm." + pname])
            h64 = torch.from_numpy(z["f64.graw." + pname]).double(); h32 = torch.from_numpy(z["graw." + pname]).double()
            ours = g.detach().reshape(-1)[:h64.numel()].double().cpu()
            print(f"{name} {pname}: norm off {abs(float(g.norm()) - r64):.2e} (own {abs(r32 - r64):.2e}), head off {float((ours - h64).norm()):.2e} (own {float((h32 - h64).norm()):.2e})")
            # the norm gate of test_gpu_pvt_b0.py takes the reference's own |norm32 - norm64| as its yardstick: a signed scalar in which the fp32 run's errors can cancel
            # (seq: lgag1.psi.0.weight 3.3e-5 against a whole-tensor distance of 6.0e-4; k333: mscb4 pconv1 2.7e-4 against >= 9.7e-3).  A norm cannot be further off
            # than the vector (| |a| - |b| | <= |a - b|), so the same band of 3 is also granted on the reference's own whole-gradient distance own.gerr
            assert abs(float(g.norm()) - r64) <= max(rel * r64, band * abs(r32 - r64), band * float(z["own.gerr." + pname])) + 2e-6, pname
            assert float((ours - h64).norm()) <= max(rel * float(h64.norm()), band * float((h32 - h64).norm())) + 2e-6, pname
    else:
        rels = [rell2(o.detach()[:, :, ::sub, ::sub], torch.from_numpy(z[f"f64.out{i}"])) for i, o in enumerate(outs)]
        print(f"\n{name} bf16, rel-L2 of the maps against the reference's float64 run:", " ".join(f"{v:.3f}" for v in rels))
        for i, v in enumerate(rels):
            assert v < 0.35, i
        assert abs(float(loss.detach()) - float(z["f64.loss"])) < 5e-2 * float(z["f64.loss"])
        for n_, p in names.items():
            if p.grad is not None:
                assert bool(torch.isfinite(p.grad).all()), n_


def test_trainer_capture_replay_all_switches():
    """Configuration `all`, bf16: capture() + two replay()s give the losses and the parameters of the same eager step()s bit for bit, and a second, fresh capture
    replays the same bits."""
    from pn2.trainer import Trainer
    _, x, label, bg = S.fixture("all")
    x, tgt = x.to(dev), (label.to(dev), bg.to(dev))

    def trainer():
        m = _model("all", "bf16")
        return Trainer(m, lr=1e-3, clip=None, weight_decay=1e-2, loss="mutation", hot=m.hot_parameters(True))
    eager = trainer()
    for _ in range(2):
        eager.step(x, tgt)
    want = [eager.step(x, tgt).clone() for _ in range(2)]
    torch.cuda.synchronize()
    runs = []
    for _ in range(2):
        cap = trainer()
        cap.capture(x, tgt, warmup=2)
        got = [cap.replay(x, tgt).clone() for _ in range(2)]
        torch.cuda.synchronize()
        runs.append((got, cap.flat.clone()))
    for got, flat in runs:
        assert all(torch.isfinite(l).all() for l in got)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert torch.equal(flat, eager.flat)
    assert torch.equal(runs[0][1], runs[1][1]) and all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))


def test_volume_predictor_all_single():
    """Configuration `all_single`, eval mode, one 4-slice volume at the patch size: the labels are the argmax of the module surface's last map."""
    import pn2
    import volevalref as VR
    from oracle import weights as W
    from pn2.infer import VolumePredictor
    pn2.set_compute_dtype("bf16")
    m = S.build("all_single")
    m.load_state_dict(VR.nontrivial_bn_stats(W.make_state_dict(S.manifest("all_single"), seed=5), seed=17), strict=True)
    m = m.to(dev).eval()
    image = torch.randn(4, 64, 64, generator=torch.Generator().manual_seed(33)).to(dev)
    with torch.no_grad():
        want = torch.cat([m(image[i:i + 2, None].contiguous())[-1].argmax(1) for i in (0, 2)]).to(torch.uint8)
    got = VolumePredictor(m, patch_size=(64, 64), batch_size=2).predict(image, "last")
    assert got.dtype == torch.uint8 and tuple(got.shape) == (4, 64, 64)
    assert torch.equal(got, want) and len(torch.unique(want)) > 1
