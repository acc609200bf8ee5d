"""CPU restatement of the reference's multi-class volume evaluation (multiclass_seg/EMCAD/utils/utils.py:140-301) for the tests of pn2.voleval:
medpy.metric.binary's dc, jc, hd95, assd and their __surface_distances with numpy + scipy.ndimage (medpy itself is a third-party dependency of the
reference), calculate_metric_percase / calculate_dice_percase on top, the label combination of test_single_volume / val_single_volume in plain numpy,
and the single-supervision EMCADNet forward from the pieces of oracle.emcad_oracle."""
import numpy as np
import torch
import torch.nn.functional as F
from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure

from oracle import emcad_oracle as E
from oracle.pranet_oracle import Ctx, bn, pvt_features


# ------------------------------------------------------------------------------------------------ medpy.metric.binary
def border(mask):
    """mask ^ binary_erosion(mask, generate_binary_structure(ndim, 1)) (border value 0): the voxels with a face neighbour outside the mask."""
    mask = np.atleast_1d(mask.astype(bool))
    return mask ^ binary_erosion(mask, structure=generate_binary_structure(mask.ndim, 1), iterations=1)


def surface_distances(result, reference):
    """__surface_distances(result, reference, voxelspacing=None, connectivity=1): the distance of every border voxel of result to the border of reference."""
    result, reference = np.atleast_1d(result.astype(bool)), np.atleast_1d(reference.astype(bool))
    if 0 == np.count_nonzero(result):
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if 0 == np.count_nonzero(reference):
        raise RuntimeError("The second supplied array does not contain any binary object.")
    dt = distance_transform_edt(~border(reference))
    return dt[border(result)]


def hd95(result, reference):
    return np.percentile(np.hstack((surface_distances(result, reference), surface_distances(reference, result))), 95)


def asd(result, reference):
    return surface_distances(result, reference).mean()


def assd(result, reference):
    return np.mean((asd(result, reference), asd(reference, result)))


def dc(result, reference):
    result, reference = np.atleast_1d(result.astype(bool)), np.atleast_1d(reference.astype(bool))
    intersection = np.count_nonzero(result & reference)
    try:
        return 2. * intersection / float(np.count_nonzero(result) + np.count_nonzero(reference))
    except ZeroDivisionError:
        return 0.0


def jc(result, reference):
    result, reference = np.atleast_1d(result.astype(bool)), np.atleast_1d(reference.astype(bool))
    return float(np.count_nonzero(result & reference)) / float(np.count_nonzero(result | reference))


# ------------------------------------------------------------------------------------------------ utils.py:140-163
def calculate_metric_percase(pred, gt):
    pred, gt = pred.copy(), gt.copy()
    pred[pred > 0] = 1
    gt[gt > 0] = 1
    if pred.sum() > 0 and gt.sum() > 0:
        return dc(pred, gt), hd95(pred, gt), jc(pred, gt), assd(pred, gt)
    elif pred.sum() > 0 and gt.sum() == 0:
        return 1, 0, 1, 0
    else:
        return 0, 0, 0, 0


def calculate_dice_percase(pred, gt):
    pred, gt = pred.copy(), gt.copy()
    pred[pred > 0] = 1
    gt[gt > 0] = 1
    if pred.sum() > 0 and gt.sum() > 0:
        return dc(pred, gt)
    elif pred.sum() > 0 and gt.sum() == 0:
        return 1
    else:
        return 0


def volume_metrics(pred, label, classes):
    return [calculate_metric_percase(pred == i, label == i) for i in range(1, classes)]          # utils.py:232-234


def volume_dice(pred, label, classes):
    return [calculate_dice_percase(pred == i, label == i) for i in range(1, classes)]            # utils.py:298-300


def d2_histogram(result, reference, length):
    """rint(dt[border]^2) of one direction as a histogram of `length` bins."""
    return np.bincount(np.rint(surface_distances(result, reference) ** 2).astype(np.int64), minlength=length)


# ------------------------------------------------------------------------------------------------ label combination (utils.py:184-195, :261-273)
def combine(outs, mode):
    """outs: fp32 arrays [N][K][H][W]; the reference's `outputs` in fp32, in its order."""
    if mode == "last":
        return outs[-1]
    if mode == "sum_fg":
        acc = np.float32(0.0)
        for p in outs:
            acc = acc + p
        return acc
    if mode == "sum_fg_minus_bg":
        h = len(outs) // 2
        acc = np.float32(0.0)
        for i in range(h):
            acc = acc + (outs[i] - outs[h + i])
        return acc
    raise ValueError(mode)


def labels(outs, mode, softmax=True):
    """argmax(softmax(outputs, dim=1), dim=1) as the reference takes it (first maximum); softmax=False: the argmax of the logits."""
    x = combine(outs, mode)
    assert x.dtype == np.float32
    t = torch.from_numpy(np.ascontiguousarray(x))
    return torch.argmax(torch.softmax(t, dim=1) if softmax else t, dim=1).numpy().astype(np.uint8)


# ------------------------------------------------------------------------------------------------ EMCADNet(dual=False) forward (networks.py:100-142, decoders.py:356-405)
def emcadnet_single_forward(P, x, training):
    """[p4, p3, p2, p1]: EMCAD decoder stages + the four biased out_head 1x1 convs + bilinear up-sampling, over a flat state_dict P."""
    ctx = Ctx(training)
    if x.shape[1] == 1:
        x = F.relu(bn(P, "conv.1", F.conv2d(x, P["conv.0.weight"], P["conv.0.bias"]), ctx))
    x1, x2, x3, x4 = pvt_features(P, "backbone.", x)
    p = "decoder."

    def stage(d, lvl):
        d = E.cab(P, p + f"cab{lvl}.", d) * d
        d = E.sab(P, p + "sab.", d) * d
        return E.mscb(P, p + f"mscb{lvl}.0.", d, ctx)
    d = stage(x4, 4)
    ds = [d]
    for lvl, skip in ((3, x3), (2, x2), (1, x1)):
        d = E.eucb(P, p + f"eucb{lvl}.", d, ctx)
        d = d + E.lgag(P, p + f"lgag{lvl}.", d, skip, ctx)
        d = stage(d, lvl)
        ds.append(d)
    ps = [F.conv2d(d, P[f"out_head{l}.weight"], P[f"out_head{l}.bias"]) for d, l in zip(ds, (4, 3, 2, 1))]
    return [F.interpolate(q, scale_factor=s, mode="bilinear") for q, s in zip(ps, (32, 16, 8, 4))]


def nontrivial_bn_stats(sd, seed):
    """A copy of state_dict sd with every BatchNorm running_mean / running_var set to non-trivial values (eval mode then differs from an identity fold)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in sd.items():
        if k.endswith("running_mean"):
            out[k] = torch.randn(v.shape, generator=g) * 0.2
        elif k.endswith("running_var"):
            out[k] = torch.rand(v.shape, generator=g) * 1.0 + 0.5
        else:
            out[k] = v.clone()
    return out
