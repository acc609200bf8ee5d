"""GPU tests of the kernels that end a PraNet-V2 training step, each on its own through the C ABI against tests/tailref.py in float64: the 31 x 31 boundary
weights (pn2_loss_weights / _clear), the dual structure loss (pn2_structure_loss_fwd / _bwd / _bwd_dev) and the optimizer step (pn2_adam_tick + pn2_clamp_adam).

Tolerance rule (the project's own, as in test_single_emcadnet_forward_backward_vs_reference): for a quantity q
    |ours - ref64| <= max(floor, 3 * |ref32 - ref64|)
where ref32 is the same tailref function run in fp32 on the CPU (the factor 3 allows for another summation order) and the floor is the bound the project already
uses for q: loss 2e-6 * max(1, |loss|) and gradients 2e-5 relmax (test_structure_loss_golden); weit 8 ulp at the top of its range [1, 6]; sums / wsum 1e-6
relative.  No bound is taken from a kernel's result; every case prints its own and ref32's distance (run with -s).  The Adam bound is derived in
test_clamp_adam_vs_float64."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import tailref as R

pytestmark = pytest.mark.gpu
dev = "cuda"

WEIT_FLOOR = 8 * 2.0 ** -23 * 6
SUM_FLOOR = 1e-6
LOSS_FLOOR = 2e-6
GRAD_FLOOR = 2e-5


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()
    yield
    pn2.set_compute_dtype("bf16")


def _lib():
    from pn2 import capi
    return capi.load()


def _p(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


# ================================================================================================================ boundary weights
def _weights(mask, ks, fill=None):
    """pn2_loss_weights on mask [N][H][W] (CPU fp32) -> (status, weit [N][H][W] on the CPU)."""
    N, H, W = mask.shape
    weit = torch.empty(N, H, W, device=dev) if fill is None else torch.full((N, H, W), fill, device=dev)
    rc = _lib().pn2_loss_weights(_p(mask.to(dev)), _p(weit), N, H, W, ks, _stream())
    torch.cuda.synchronize()
    return rc, weit.cpu()


def _check_weit(tag, mask, ks):
    rc, ours = _weights(mask, ks)
    assert rc == 0, rc
    ref64 = R.weights_ref(mask.double(), ks)
    d32 = float((R.weights_ref(mask, ks).double() - ref64).abs().max())
    d = float((ours.double() - ref64).abs().max())
    print(f"\nTAILK weit {tag} ks={ks}: ours {d:.2e} ref32 {d32:.2e}")
    assert d <= max(WEIT_FLOOR, 3 * d32)
    return ours


@pytest.mark.parametrize("kind", R.WEIGHT_KINDS)
@pytest.mark.parametrize("shape", R.WEIGHT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_loss_weights_vs_float64(shape, kind):
    """ks = 31 over the tile geometry of loss_weights_k (32 x 64 tiles, 16-column / 8-row sliding segments, a halo of 15): window larger than the image, one below /
    exactly / one past a tile, 3 x 3 tiles with a ragged edge, a single column segment; binary, constant and soft masks, three images."""
    ours = _check_weit(f"{shape[0]}x{shape[1]} {kind}", R.weight_masks(kind, *shape), 31)
    if kind == "zeros":
        assert torch.equal(ours, torch.ones_like(ours))


@pytest.mark.parametrize("kind", ["blob", "soft"])
@pytest.mark.parametrize("ks", R.WEIGHT_KS)
def test_loss_weights_other_window_sizes(ks, kind):
    ours = _check_weit(f"33x65 {kind}", R.weight_masks(kind, 33, 65), ks)
    if ks == 1:
        assert torch.equal(ours, torch.ones_like(ours))


@pytest.mark.parametrize("ks", [0, 2, 65])
def test_loss_weights_rejects_window(ks):
    mask = R.weight_masks("blob", 33, 65)
    rc, out = _weights(mask, ks, fill=7.0)
    assert rc == -2 and torch.equal(out, torch.full_like(out, 7.0))
    weit = torch.full((3, 33, 65), 7.0, device=dev)
    clr = torch.full((8,), -1, dtype=torch.int64, device=dev)
    assert _lib().pn2_loss_weights_clear(_p(mask.to(dev)), _p(weit), 3, 33, 65, ks, _p(clr), 8, _stream()) == -2
    torch.cuda.synchronize()
    assert torch.equal(weit.cpu(), torch.full((3, 33, 65), 7.0)) and bool((clr == -1).all())


@pytest.mark.parametrize("shape", [(33, 65), (70, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_loss_weights_clear(shape):
    """The launch that also zeroes the image-sum accumulators: same weit bit for bit, exactly `nclear` 64-bit words cleared, nclear = 0 / NULL accepted."""
    H, W = shape
    mask = R.weight_masks("soft", H, W)
    rc, want = _weights(mask, 31)
    assert rc == 0
    md = mask.to(dev)
    weit = torch.empty(3, H, W, device=dev)
    clr = torch.full((338,), -1, dtype=torch.int64, device=dev)
    assert _lib().pn2_loss_weights_clear(_p(md), _p(weit), 3, H, W, 31, _p(clr), 330, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(weit.cpu(), want)
    assert bool((clr[:330] == 0).all()) and bool((clr[330:] == -1).all())
    weit2 = torch.empty(3, H, W, device=dev)
    assert _lib().pn2_loss_weights_clear(_p(md), _p(weit2), 3, H, W, 31, C.c_void_p(0), 0, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(weit2.cpu(), want)


# ================================================================================================================ structure loss
@functools.lru_cache(maxsize=None)
def _loss_refs(name):
    """float64 and fp32 references of a case on the kernel's own weit (kept by _loss_run)."""
    fg, bg, mask = R.loss_case(name)
    weit = _loss_run(name)["weit_cpu"]
    return tuple(R.structure_loss_ref(list(fg.to(dt)), list(bg.to(dt)), mask.to(dt), weit=weit.to(dt), grad=True) for dt in (torch.float64, torch.float32))


@functools.lru_cache(maxsize=None)
def _loss_run(name):
    """weit, forward and backward of a case through the C ABI, once per session."""
    from pn2.loss import loss_backward, loss_forward
    P, N, H, W, _ = R.LOSS_CASES[name]
    fg, bg, mask = R.loss_case(name)
    HW = H * W
    buf = torch.cat([fg, bg]).reshape(2 * P, N, HW).contiguous().to(dev)
    md = mask.reshape(N, HW).to(dev)
    loss, saved = loss_forward(buf, P, md, N, HW, H, W)
    dbuf = torch.full_like(buf, float("nan"))
    loss_backward(buf, dbuf, P, md, saved, N, HW)
    torch.cuda.synchronize()
    weit, sums, wsum = saved
    return dict(buf=buf, mask=md, saved=saved, dbuf=dbuf, loss=loss.cpu(), sums=sums.cpu(), wsum=wsum.cpu(), weit_cpu=weit.cpu().reshape(N, H, W), dims=(P, N, H, W))


def _assert_grads(tag, dbuf, ref64, ref32, P, N, H, W, skip=()):
    worst = (0.0, 0.0)
    for j in range(2 * P):
        p, key = j % P, "gfg" if j < P else "gbg"
        ours = dbuf[j].reshape(N, H, W)
        assert bool(torch.isfinite(ours).all()), (tag, j)
        if p in skip:
            continue
        d, d32 = relmax(ours, ref64[key][p]), relmax(ref32[key][p], ref64[key][p])
        worst = max(worst, (d, d32))
        assert d <= max(GRAD_FLOOR, 3 * d32), (tag, j, d, d32)
    print(f"TAILK lossgrad {tag}: ours {worst[0]:.2e} ref32 {worst[1]:.2e}")


@pytest.mark.parametrize("name", list(R.LOSS_CASES))
def test_structure_loss_vs_float64(name):
    """Per-pair losses, their total, sums, wsum and both gradient maps of every pair, on the kernel's own weit (itself held to float64 here as well)."""
    r = _loss_run(name)
    P, N, H, W = r["dims"]
    fg, bg, mask = R.loss_case(name)
    dw = float((r["weit_cpu"].double() - R.weights_ref(mask.double(), 31)).abs().max())
    assert dw <= max(WEIT_FLOOR, 3 * float((R.weights_ref(mask, 31).double() - R.weights_ref(mask.double(), 31)).abs().max()))
    ref64, ref32 = _loss_refs(name)
    ours = r["loss"].double()
    assert bool(torch.isfinite(ours).all())
    want = torch.cat([ref64["losses"], ref64["total"][None]])
    want32 = torch.cat([ref32["losses"], ref32["total"][None]]).double()
    d, d32 = (ours - want).abs(), (want32 - want).abs()
    print(f"\nTAILK loss {name}: ours {float((d / want.abs().clamp(min=1)).max()):.2e} ref32 {float((d32 / want.abs().clamp(min=1)).max()):.2e}")
    assert bool((d <= torch.maximum(LOSS_FLOOR * want.abs().clamp(min=1), 3 * d32)).all()), (d, d32)
    for key, got in (("sums", r["sums"]), ("wsum", r["wsum"])):
        w64, w32 = ref64[key], ref32[key].double()
        d, d32 = (got.double() - w64).abs(), (w32 - w64).abs()
        den = w64.abs().clamp(min=1e-300)
        print(f"TAILK {key} {name}: ours {float((d / den).max()):.2e} ref32 {float((d32 / den).max()):.2e}")
        assert bool((d <= torch.maximum(SUM_FLOOR * w64.abs(), 3 * d32)).all()), (key, d / den, d32 / den)
    _assert_grads(name, r["dbuf"].cpu(), ref64, ref32, P, N, H, W)


def _bwd_dev(r, dmap_stride, gdev, gscale, fill=7.0):
    P, N, H, W = r["dims"]
    HW = H * W
    weit, sums, wsum = r["saved"]
    out = torch.full((2 * P * dmap_stride,), fill, device=dev)
    rc = _lib().pn2_structure_loss_bwd_dev(_p(r["buf"]), _p(out), N * HW, dmap_stride, P, _p(r["mask"]), _p(weit), _p(wsum), _p(sums), _p(gdev), gscale, N, HW, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return out.reshape(2 * P, dmap_stride).cpu()


def test_structure_loss_bwd_dev_equals_bwd():
    """gscale_dev = NULL: the same gradient bit for bit, at the forward's map stride and at a stride of its own whose 24-float gaps are not written."""
    r = _loss_run("p4n3_20x27")
    P, N, H, W = r["dims"]
    want = r["dbuf"].cpu().reshape(2 * P, N * H * W)
    assert torch.equal(_bwd_dev(r, N * H * W, None, 1.0), want)
    out = _bwd_dev(r, N * H * W + 24, None, 1.0)
    assert torch.equal(out[:, :N * H * W], want)
    assert torch.equal(out[:, N * H * W:], torch.full((2 * P, 24), 7.0))


def test_structure_loss_bwd_dev_upstream_gradients():
    """Per-pair upstream gradients read from the device, times a global scale: the float64 gradient of 0.5 * sum_p u[p] * loss[p]; the pair with u = 0 gets zeros."""
    r = _loss_run("p4n3_20x27")
    P, N, H, W = r["dims"]
    fg, bg, mask = R.loss_case("p4n3_20x27")
    gdev = torch.tensor(R.UPSTREAM, device=dev)
    out = _bwd_dev(r, N * H * W + 24, gdev, R.UPSTREAM_SCALE)
    refs = [R.structure_loss_ref(list(fg.to(dt)), list(bg.to(dt)), mask.to(dt), weit=r["weit_cpu"].to(dt), upstream=R.UPSTREAM, gscale=R.UPSTREAM_SCALE, grad=True)
            for dt in (torch.float64, torch.float32)]
    zero = [p for p, u in enumerate(R.UPSTREAM) if u == 0]
    print()
    _assert_grads("bwd_dev upstream", out[:, :N * H * W], refs[0], refs[1], P, N, H, W, skip=zero)
    for p in zero:
        assert int(torch.count_nonzero(out[p, :N * H * W])) == 0 and int(torch.count_nonzero(out[P + p, :N * H * W])) == 0
    assert torch.equal(out[:, N * H * W:], torch.full((2 * P, 24), 7.0))


@pytest.mark.parametrize("P,N", [(9, 1), (8, 65)])
def test_structure_loss_rejects_pair_counts(P, N):
    HW = 35
    buf = torch.zeros(2 * P, N, HW, device=dev)
    mask, weit = torch.zeros(N, HW, device=dev), torch.ones(N, HW, device=dev)
    partial, sums, wsum = torch.zeros(P, N, 1, 5, device=dev), torch.zeros(P, N, 4, device=dev), torch.zeros(N, device=dev)
    loss = torch.full((P + 1,), 7.0, device=dev)
    rc = _lib().pn2_structure_loss_fwd(_p(buf), N * HW, P, _p(mask), _p(weit), _p(partial), _p(sums), _p(wsum), _p(loss), N, HW, _stream())
    torch.cuda.synchronize()
    assert rc == -2 and bool((loss == 7.0).all())


# ================================================================================================================ clamp + Adam
HP = {k: R.f32(v) for k, v in R.ADAM_HP.items()}          # the constants as the C ABI's `float` arguments carry them, for the kernel and the reference alike


def _bc(dev_block=None):
    bc = torch.tensor([0, 0, 1, 1, 0, 0, 0, 0], dtype=torch.float32)
    if dev_block is not None:
        bc[4:7] = torch.tensor(dev_block, dtype=torch.float32)
        bc[7] = 1
    return bc.to(dev)


def _adam_step(p, g, m, v, n, bc, lr, clip, gscale, wd, offsets=(0, 0, 0, 0)):
    lib = _lib()
    assert lib.pn2_adam_tick(_p(bc), HP["b1"], HP["b2"], _stream()) == 0
    rc = lib.pn2_clamp_adam(_p(p, offsets[0]), _p(g, offsets[1]), _p(m, offsets[2]), _p(v, offsets[3]), n, lr, HP["b1"], HP["b2"], HP["eps"], clip, gscale, _p(bc), wd, _stream())
    torch.cuda.synchronize()
    return rc


def _buffers(n, p0):
    """Four device buffers of n floats behind a never-written guard of 4 (n = 0 still needs valid pointers)."""
    bufs = [torch.full((n + 4,), 7.0, device=dev) for _ in range(4)]
    bufs[0][:n] = p0.to(dev)
    bufs[2][:n] = 0
    bufs[3][:n] = 0
    return bufs


@pytest.mark.parametrize("wd", R.ADAM_WD)
@pytest.mark.parametrize("clipname", list(R.ADAM_CLIPS))
@pytest.mark.parametrize("n", R.ADAM_N)
def test_clamp_adam_vs_float64(n, clipname, wd):
    """T = 5 consecutive steps (tick, then update) against adam_ref in float64, checked after every step.

    g: exactly clamp(g0 * gscale, +-clip) of fp32 torch.  m, v: 1e-6 relmax (T steps of two fp32 roundings each).  p: the update is
    dp = (lr / bc0) * m / (sqrt(v) / sqrt(bc1) + eps) with the bias corrections bc0 = 1 - b1^t, bc1 = 1 - b2^t that the device builds by repeated fp32
    multiplication (adam_tick_k), so dp inherits rel(bc0_t) + rel(bc1_t) / 2, which tailref.bias_corr_rel_err follows from the constants alone, plus the roundings
    of its own few operations (8 * 2^-24); p itself is rounded once per step (and once more for the decay factor):
        |p_t - p64_t| <= sum_{s<=t} rho_s * |dp64_s| + t * 2^-23 * |p64_t|,   rho_s = rel(bc0_s) + rel(bc1_s) / 2 + 8 * 2^-24.
    The reference works on the fp32 values of lr, betas, eps, clip, wd that the entry point receives."""
    clip, gscale = (R.f32(x) for x in R.ADAM_CLIPS[clipname])
    wd = R.f32(wd)
    p0, grads = R.adam_case(n)
    p, g, m, v = _buffers(n, p0)
    bc = _bc()
    e0, e1 = R.bias_corr_rel_err(HP["b1"], R.ADAM_T), R.bias_corr_rel_err(HP["b2"], R.ADAM_T)
    p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    acc = torch.zeros(n, dtype=torch.float64)
    worst = dict(p=0.0, m=0.0, v=0.0)
    for t in range(1, R.ADAM_T + 1):
        g[:n] = grads[t - 1].to(dev)
        assert _adam_step(p, g, m, v, n, bc, HP["lr"], clip, gscale, wd) == 0
        for b in (p, g, m, v):
            assert bool((b[n:] == 7.0).all())
        if n == 0:
            continue
        prev = p64
        p64, g64, m64, v64 = R.adam_ref(p64, grads[t - 1], m64, v64, t, HP["lr"], HP["b1"], HP["b2"], HP["eps"], clip, gscale, wd)
        assert torch.equal(g[:n].cpu(), (grads[t - 1] * gscale).clamp(-clip, clip))
        worst["m"], worst["v"] = max(worst["m"], relmax(m[:n], m64)), max(worst["v"], relmax(v[:n], v64))
        assert relmax(m[:n], m64) <= 1e-6 and relmax(v[:n], v64) <= 1e-6, t
        acc += (e0[t - 1] + 0.5 * e1[t - 1] + 8 * 2.0 ** -24) * (p64 - prev * (1 - HP["lr"] * wd)).abs()
        bound = acc + t * 2.0 ** -23 * p64.abs()
        ratio = float(((p[:n].cpu().double() - p64).abs() / bound).max())
        worst["p"] = max(worst["p"], ratio)
        assert ratio <= 1.0, t
    print(f"\nTAILK adam n={n} {clipname} wd={wd:g}: p error/bound {worst['p']:.3f} m relmax {worst['m']:.2e} v relmax {worst['v']:.2e}")


def _adam_run(n, lrs, clip, gscale, wd, dev_block):
    """Steps with the given learning rates; dev_block: lr / clip / wd through bc[4..7] and deliberately different ones as arguments."""
    p0, grads = R.adam_case(n)
    p, g, m, v = _buffers(n, p0)
    bc = _bc((lrs[0], clip, wd) if dev_block else None)
    out = []
    for t, lr in enumerate(lrs):
        g[:n] = grads[t].to(dev)
        if dev_block:
            bc[4] = lr
            assert _adam_step(p, g, m, v, n, bc, 1.0, 1e-3, gscale, 0.5) == 0
        else:
            assert _adam_step(p, g, m, v, n, bc, lr, clip, gscale, wd) == 0
        out.append([b.cpu().clone() for b in (p, g, m, v)])
    return out


def test_clamp_adam_device_block():
    """bc[7] = 1: lr, clip and weight decay are read from bc[4..6] and the arguments are ignored - bit for bit the argument-driven run; a new bc[4] is the next
    step's learning rate."""
    clip, gscale = (R.f32(x) for x in R.ADAM_CLIPS["clip"])
    wd, lr = R.f32(1e-2), HP["lr"]
    lrs = [lr, R.f32(2 * lr), R.f32(0.5 * lr)]
    args = _adam_run(1023, lrs, clip, gscale, wd, False)
    block = _adam_run(1023, lrs, clip, gscale, wd, True)
    for a, b in zip(args, block):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    const = _adam_run(1023, [lr, lr, lr], clip, gscale, wd, True)
    assert torch.equal(const[0][0], block[0][0]) and not torch.equal(const[1][0], block[1][0])


@pytest.mark.parametrize("wd", R.ADAM_WD)
def test_clamp_adam_zero_gradient(wd):
    """g = m = v = 0: without decay p keeps its bits; with decay it is p * (1 - lr * wd) in fp32 exactly.  Moments and gradient stay zero."""
    n, wd = 1023, R.f32(wd)
    p0, _ = R.adam_case(n)
    p, g, m, v = _buffers(n, p0)
    g[:n] = 0
    bc = _bc()
    keep = np.float32(1) - np.float32(HP["lr"]) * np.float32(wd)
    want = p0.clone()
    for t in range(2):
        assert _adam_step(p, g, m, v, n, bc, HP["lr"], R.f32(0.5), 1.0, wd) == 0
        want = want * torch.tensor(keep) if wd else want
        assert torch.equal(p[:n].cpu(), want)
        for b in (g, m, v):
            assert int(torch.count_nonzero(b[:n])) == 0


@pytest.mark.parametrize("which", range(4))
def test_clamp_adam_rejects_misaligned_pointer(which):
    p0, grads = R.adam_case(5)
    bufs = _buffers(5, p0)
    bufs[1][:5] = grads[0].to(dev)
    before = [b.cpu().clone() for b in bufs]
    bc = _bc()
    off = [0, 0, 0, 0]
    off[which] = 4
    assert _adam_step(*bufs, 4, bc, HP["lr"], R.f32(0.5), 1.0, 0.0, offsets=tuple(off)) == -2
    for b, w in zip(bufs, before):
        assert torch.equal(b.cpu(), w)
