"""CPU checks of the dual-supervision loss for 2..9 classes and every supervision mode: the float64 restatement (tests/duallossref.py) against the oracle's
K = 9 / mutation form and against the losses the reference recorded at K = 4, the subsets and masks of the three modes, the refusals of the new entry points."""
import pytest
import torch

import duallossref as D
import seglossref as R


def _case(K, seed=1, N=2, H=6, W=7):
    g = torch.Generator().manual_seed(seed)
    outs = [torch.randn(N, K, H, W, generator=g, dtype=torch.float64) * 1.5 for _ in range(8)]
    label = torch.randint(0, K, (N, H, W), generator=g)
    return outs, label, D.bg_mask_of(label, K).double()


def test_restatement_equals_oracle_mutation_loss_at_k9():
    from oracle import emcad_oracle as E
    outs, label, bg = _case(9)
    got, want = float(D.dual_loss_ref(outs, label, bg)), float(E.mutation_loss(outs, label, bg))
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)


def test_modes_pick_their_subsets_and_masks():
    from pn2.loss import SEG_SUBSETS
    assert R.subsets("deep_supervision") == [(0,), (1,), (2,), (3,)] and R.subsets("last") == [(3,)]
    assert len(R.subsets("mutation")) == 15
    assert {m: R.subset_mask(m) for m in D.MODES} == SEG_SUBSETS
    # the value of each mode is the sum of the single-subset terms it names: 'last' scores maps 3 and 7 only, 'deep_supervision' is four such terms
    outs, label, bg = _case(4, seed=2)
    lc = (0.4, 0.9, 0.2)
    one = lambda i: float(D.dual_loss_ref([outs[i]] * 4 + [outs[4 + i]] * 4, label, bg, "last", lc))
    assert abs(float(D.dual_loss_ref(outs, label, bg, "last", lc)) - one(3)) <= 1e-12 * one(3)
    ds = float(D.dual_loss_ref(outs, label, bg, "deep_supervision", lc))
    assert abs(ds - sum(one(i) for i in range(4))) <= 1e-12 * ds
    with pytest.raises(ValueError):
        D.dual_loss_ref(outs, label, bg, "powerset")
    with pytest.raises(ValueError):
        D.dual_loss_ref(outs[:7], label, bg)


@pytest.mark.parametrize("mode", D.MODES)
def test_restatement_reproduces_reference_losses_at_k4(mode):
    """dual_loss_ref on the reference's float64 outputs (dual EMCADNet, pvt_v2_b0, K = 4) against the loss the reference's own trainer code computed from them."""
    z = D.load_fixture()
    outs = D.fixture_outs(z, "f64.")
    assert len(outs) == 8 and all(o.dtype == torch.float64 and tuple(o.shape) == (2, 4, 64, 64) for o in outs)
    label = torch.from_numpy(z["label"]).long()
    got, want = float(D.dual_loss_ref(outs, label, D.bg_mask_of(label, 4).double(), mode)), float(z["f64.loss." + mode])
    assert abs(got - want) <= 1e-10 * abs(want), (mode, got, want)


def test_fixture_is_data_only_and_small():
    import os
    z = D.load_fixture()
    assert sorted(z.files) == sorted(["x", "label", "scales"] + [f"{p}head{i}" for p in ("", "f64.") for i in range(8)]
                                     + [f"{p}loss.{m}" for p in ("", "f64.") for m in D.MODES])
    assert os.path.getsize(os.path.join(D.G, "emcad_dual_k4_64.npz")) <= os.path.getsize(os.path.join(D.G, "emcad_single_64.npz"))


def test_dual_manifest_matches_the_model():
    import os
    os.environ.setdefault("PN2_NO_PRETRAINED", "1")
    from lib.networks import EMCADNet
    m = EMCADNet(num_classes=4, activation="relu6", encoder="pvt_v2_b0", pretrain=False, dual=True)
    assert [(k, list(v.shape)) for k, v in m.state_dict().items()] == [(k, list(v)) for k, v in D.manifest_b0(4).items()]


def test_dual_loss_entry_points_refuse_bad_arguments_before_any_launch():
    """Status -2 for subsets == 0, a bit above 15 and K outside 2..9; -1 for a null pointer; the width helper's range.  Every case returns on a host-side check;
    the K = 9 entry points keep their own range."""
    import ctypes as C
    from pn2 import capi
    lib = capi.load()
    assert [lib.pn2_dual_loss_width(k) for k in range(0, 12)] == [-1, -1] + [15 * (2 + 2 * k) + k for k in range(2, 10)] + [-1, -1]
    assert lib.pn2_dual_loss_width(9) == lib.pn2_mutation_loss_width(9) and lib.pn2_mutation_loss_width(4) == -1
    buf = (C.c_float * 16)()
    ptr = C.cast(buf, C.c_void_p)
    four = (C.c_void_p * 4)(*[ptr.value] * 4)
    fwd = lambda subsets, K, fg=four, bg=four: lib.pn2_dual_loss_fwd(fg, bg, subsets, ptr, ptr, 1, 16, K, 0.5, 0.7, 0.3, ptr, ptr, ptr, None)
    bwd = lambda subsets, K, d=four, e=four: lib.pn2_dual_loss_bwd(four, four, d, e, subsets, ptr, ptr, 1, 16, K, 0.5, 0.7, 0.3, ptr, 1.0, None)
    for subsets, K in ((0, 9), (0x8000, 9), (0xFFFF, 4), (0x7FFF, 1), (0x7FFF, 10), (0x80, 0)):
        assert fwd(subsets, K) == -2 and bwd(subsets, K) == -2, (subsets, K)
    hole = (C.c_void_p * 4)(ptr.value, ptr.value, None, ptr.value)
    assert fwd(0x7FFF, 9, None) == -1 and fwd(0x7FFF, 9, four, None) == -1 and bwd(0x7FFF, 9, None) == -1 and bwd(0x7FFF, 9, four, None) == -1
    assert fwd(0, 9, hole) == -2 and fwd(0x7FFF, 4, hole) == -1 and fwd(0x7FFF, 4, four, hole) == -1
    assert bwd(0x7FFF, 4, hole) == -1 and bwd(0x7FFF, 4, four, hole) == -1
