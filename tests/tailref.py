"""Plain torch / numpy references (CPU) of the three kernel families that end a PraNet-V2 training step - the 31 x 31 boundary weights, the dual structure
loss and the fused clamp + Adam update - and the seeded inputs of tests/test_gpu_train_tail_kernels.py.  Nothing here is shared with the product.  Every
reference keeps the dtype of its inputs: float64 inputs give the yardstick, fp32 inputs give "the same formula in fp32" whose distance to float64 sets the
tolerance (tests/test_tailref_cpu.py checks the references against torch's own ops and the properties of the inputs the GPU tests rely on)."""
import numpy as np
import torch
import torch.nn.functional as F


def f32(x):
    """The value a `float` argument of the C ABI carries: x rounded to fp32, as a Python float.  The references get their scalars through this, so that a
    float64 reference and a kernel work on the SAME constants (0.999 is not an fp32 number; 1 - fl32(0.999) differs from 0.001 by 1.3e-5 relative)."""
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------------------- boundary weights
def weights_ref(mask, ks):
    """mask [N][H][W] -> 1 + 5 * |avg_pool2d(mask, ks, 1, ks // 2) - mask|, zero padding counted in the mean (MyTrain_med.py:21 has ks = 31)."""
    m = mask[:, None]
    return (1 + 5 * (F.avg_pool2d(m, ks, 1, ks // 2, count_include_pad=True) - m).abs())[:, 0]


# ---------------------------------------------------------------------------------------------------------------- structure loss
def structure_loss_ref(preds_fg, preds_bg, mask, weit=None, upstream=None, gscale=1.0, grad=False):
    """The dual structure loss of oracle/pranet_oracle.py:structure_loss for P (fg, bg) pairs that share one mask.

    preds_fg, preds_bg: P logit maps [N][H][W] each; mask [N][H][W]; weit: the boundary weights when the caller has them (the GPU tests hand in the kernel's),
    else weights_ref(mask, 31).  Returns a dict: per-pair `losses` [P], their `total`, `sums` [P][N][4] = (sum w*bce_fg, sum w*bce_bg, sum p*m*w,
    sum (p+m)*w), `wsum` [N]; with grad=True also `gfg`, `gbg`: the gradients of gscale * sum_p upstream[p] * losses[p] (upstream defaults to ones)."""
    P = len(preds_fg)
    dt = mask.dtype
    if weit is None:
        weit = weights_ref(mask, 31)
    fg = [x.detach().clone().requires_grad_(grad) for x in preds_fg]
    bg = [x.detach().clone().requires_grad_(grad) for x in preds_bg]
    wsum = weit.sum(dim=(1, 2))
    losses, sums = [], []
    for p in range(P):
        sf = (weit * F.binary_cross_entropy_with_logits(fg[p], mask, reduction="none")).sum(dim=(1, 2))
        sb = (weit * F.binary_cross_entropy_with_logits(bg[p], 1 - mask, reduction="none")).sum(dim=(1, 2))
        pr = torch.sigmoid(fg[p])
        inter = ((pr * mask) * weit).sum(dim=(1, 2))
        union = ((pr + mask) * weit).sum(dim=(1, 2))
        wiou = 1 - (inter + 1) / (union - inter + 1)
        losses.append((sf / wsum + wiou + 0.8 * (sb / wsum)).mean())
        sums.append(torch.stack([sf, sb, inter, union], dim=1))
    losses = torch.stack(losses)
    out = {"losses": losses.detach(), "total": losses.sum().detach(), "sums": torch.stack(sums).detach(), "wsum": wsum.detach()}
    if grad:
        up = torch.ones(P, dtype=dt) if upstream is None else torch.as_tensor(upstream, dtype=dt)
        (gscale * (up * losses).sum()).backward()
        out["gfg"] = [x.grad for x in fg]
        out["gbg"] = [x.grad for x in bg]
    return out


# ---------------------------------------------------------------------------------------------------------------- clamp + Adam
def adam_ref(p, g, m, v, t, lr, b1, b2, eps, clip, gscale, wd):
    """Step t (1-based) of the fused update in float64: g <- clamp(g * gscale, +-clip), then torch.optim.Adam (wd = 0) / torch.optim.AdamW (decoupled decay)
    with the exact bias corrections 1 - b^t.  Returns new (p, g, m, v); the inputs are not modified."""
    p, g, m, v = (x.double() for x in (p, g, m, v))
    g = (g * gscale).clamp(-clip, clip)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    p = p * (1 - lr * wd) - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps)
    return p, g, m, v


def bias_corr_rel_err(b, T):
    """Relative error of the fp32 bias correction the optimizer keeps on the device, against the exact 1 - b^t, for t = 1..T.  The device forms b^t by
    repeated fp32 multiplication (bt <- fl32(bt * b), bc <- fl32(1 - bt)); this follows it from the constant alone."""
    b = np.float32(b)
    bt, out = np.float32(1), []
    for t in range(1, T + 1):
        bt = np.float32(bt * b)
        exact = 1.0 - float(b) ** t
        out.append(abs(float(np.float32(np.float32(1) - bt)) - exact) / exact)
    return out


# ---------------------------------------------------------------------------------------------------------------- inputs of the GPU tests
def _gen(*key):
    return torch.Generator().manual_seed(int(np.prod([k + 17 for k in key]) % (2 ** 31)))


def blob_masks(N, H, W, seed=0):
    """N different binary masks [N][H][W] fp32: an ellipse somewhere inside plus a rectangle that touches the lower right corner (the zero padding of the box
    filter meets foreground there)."""
    g = _gen(N, H, W, seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    out = torch.zeros(N, H, W)
    for n in range(N):
        r = torch.rand(4, generator=g)
        cy, cx = (0.25 + 0.5 * float(r[0])) * H, (0.25 + 0.5 * float(r[1])) * W
        ry, rx = (0.15 + 0.2 * float(r[2])) * H + 1, (0.15 + 0.2 * float(r[3])) * W + 1
        out[n] = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1).float()
        out[n, H - 1 - H // 6:, W - 1 - W // 5 - n:] = 1.0
    return out


WEIGHT_SHAPES = [(7, 9), (31, 63), (32, 64), (33, 65), (70, 130), (40, 16)]     # against the 32 x 64 tile, 16-column / 8-row segments of loss_weights_k
WEIGHT_KINDS = ["blob", "zeros", "ones", "soft"]
WEIGHT_KS = [1, 3, 63]                                                          # at (33, 65), besides the 31 of the loss


def weight_masks(kind, H, W, N=3):
    if kind == "blob":
        return blob_masks(N, H, W)
    if kind == "zeros":
        return torch.zeros(N, H, W)
    if kind == "ones":
        return torch.ones(N, H, W)
    assert kind == "soft"          # what multi-scale training feeds: a bilinearly resized ground truth takes every value in [0, 1]
    return torch.rand(N, H, W, generator=_gen(N, H, W, 5))


# name -> (P, N, H, W, variant)
LOSS_CASES = {
    "p1n1_5x7": (1, 1, 5, 7, "randn"),                  # HW = 35: one partial wave
    "p4n3_20x27": (4, 3, 20, 27, "randn"),              # HW = 540: two full passes of a 256-thread block and a partial one
    "p4n2_96x90": (4, 2, 96, 90, "randn"),              # HW = 8640: 3 chunks of 2880 (chunk starts off the 256 grid); 9 backward blocks
    "p8n2_33x65": (8, 2, 33, 65, "randn"),              # the P limit
    "p1n1_520x512": (1, 1, 520, 512, "randn"),          # HW = 266240: 65 chunks clamped to 64; 260 backward blocks clamped to 256 (grid stride)
    "saturated": (4, 3, 20, 27, "saturated"),
    "const_masks": (4, 3, 20, 27, "const_masks"),
    "soft_mask": (4, 3, 20, 27, "soft_mask"),
}


def loss_case(name):
    """-> (fg [P][N][H][W], bg [P][N][H][W], mask [N][H][W]), fp32.  Logits are randn * 3 except in the `saturated` variant."""
    P, N, H, W, variant = LOSS_CASES[name]
    g = _gen(P, N, H, W, len(name))
    fg, bg = torch.randn(P, N, H, W, generator=g) * 3, torch.randn(P, N, H, W, generator=g) * 3
    mask = blob_masks(N, H, W, seed=1)
    if variant == "const_masks":          # one empty and one full ground truth next to a blob
        mask[1], mask[2] = 0.0, 1.0
    elif variant == "soft_mask":
        mask = torch.rand(N, H, W, generator=g)
    elif variant == "saturated":
        # every 4th pixel carries a logit of magnitude 40 or 100 whose sign agrees or disagrees with its target (fg: mask, bg: 1 - mask), all four combinations
        i = torch.arange(H * W).reshape(H, W)
        sat = (i % 4 == 0)
        mag = torch.where((i // 4) % 2 == 0, 40.0, 100.0)
        agree = torch.where((i // 8) % 2 == 0, 1.0, -1.0)
        sgn = 2 * mask - 1
        fg = torch.where(sat, mag * agree * sgn[None], fg)
        bg = torch.where(sat, -mag * agree * sgn[None], bg)
    return fg.contiguous(), bg.contiguous(), mask.contiguous()


UPSTREAM = [1.5, 0.0, -2.0, 0.25]          # per-pair upstream gradients of the pn2_structure_loss_bwd_dev test (P = 4), times a global 0.5
UPSTREAM_SCALE = 0.5

ADAM_T = 5
ADAM_N = [0, 1, 3, 4, 5, 1023, 4 * 4096 * 256 + 4 * 1024 + 3]      # float4 body / scalar tail of n mod 4 / more float4s than 4096 blocks x 256 threads
ADAM_CLIPS = {"clip": (0.5, 0.25), "noclip": (3.0e38, 1.0)}       # name -> (clip, gscale)
ADAM_WD = [0.0, 1e-2]
ADAM_HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def adam_case(n):
    """-> (p0 [n], grads [T][n]) fp32: parameters randn, raw gradients randn * 0.8 (a new one every step).  With gscale = 0.25 and clip = 0.5 only 1.2 % of
    such elements are clamped, none at all in the small cases: every other step one element is set to +-2.4 (0.6 after scaling), so that each case has clamped
    and unclamped elements whatever its size."""
    g = _gen(n % 100003, 3)
    p0, grads = torch.randn(n, generator=g), torch.randn(ADAM_T, n, generator=g) * 0.8
    for t in range(0, ADAM_T if n else 0, 2):
        grads[t, t % n] = 2.4 if t % 4 == 0 else -2.4
    return p0, grads
