"""The ResNet encoders of EMCADNet on the CPU: the mirror builds with the reference's state_dict layout (tests/golden/make_golden_emcad_resnet.py), its 1000-way head
stays out of the trained parameters, pretrained weights only ever come from disk, and the two entry points of csrc/pn2_resnet.hip refuse bad arguments on the host."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pranet-v2_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("PN2_NO_PRETRAINED", "1")
import emcad_resnetref as R  # noqa: E402


def test_emcadnet_resnet50_state_dict_matches_reference_manifest():
    m = R.build("resnet50")
    ref = R.reference_manifest()
    assert [(k, list(v.shape)) for k, v in m.state_dict().items()] == list(ref.items())
    assert sum(p.numel() for p in m.parameters()) == R.manifests()["n_params"]
    assert [len(l) for l in (m.backbone.layer1, m.backbone.layer2, m.backbone.layer3, m.backbone.layer4)] == [3, 4, 6, 3]
    assert [m.backbone.layer1[0].downsample[0].stride, m.backbone.layer2[0].downsample[0].stride] == [(1, 1), (2, 2)]
    assert m.out_head4.in_channels == 2048 and m.out_head1.in_channels == 256


@pytest.mark.parametrize("name", ["resnet101", "resnet152"])
def test_deeper_backbones_match_reference_key_lists(name):
    from lib import resnet
    got = [[k, list(v.shape)] for k, v in getattr(resnet, name)().state_dict().items()]
    assert got == R.manifests()[name]


def test_hot_parameters_exclude_the_classifier_head():
    m = R.build("resnet50")
    names = {id(p): n for n, p in m.named_parameters()}
    hot = {names[id(p)] for p in m.hot_parameters()}
    assert "backbone.fc.weight" in names.values() and "backbone.fc.bias" in names.values()
    assert not any(n.startswith("backbone.fc.") for n in hot)
    assert {"backbone.conv1.weight", "backbone.layer4.2.bn3.weight", "backbone.layer2.0.downsample.0.weight", "conv.0.weight", "decoder.mscb4.0.pconv1.0.weight"} <= hot
    assert not any(n.startswith("out_head") for n in hot)                                  # dual: as for the PVTv2 encoders
    single = R.build("resnet101", dual=False)
    sn = {id(p): n for n, p in single.named_parameters()}
    assert {sn[id(p)] for p in single.hot_parameters()} == {n for n in sn.values() if not n.startswith("backbone.fc.")}
    assert [n for n, _ in m.backbone.named_parameters() if n.startswith("fc.")] == ["fc.weight", "fc.bias"]
    assert len(m.backbone.hot_parameters()) == len(list(m.backbone.parameters())) - 2


def test_pretrain_without_a_file_builds_offline(monkeypatch, tmp_path):
    """pretrain=True, no ./pretrained_pth/resnet/resnet50.pth, PN2_NO_PRETRAINED=1: random init, and nothing reaches for the network."""
    import socket
    import torch
    import lib.resnet as mirror

    def refuse(*a, **k):
        raise AssertionError("the constructor touched the network")
    monkeypatch.setattr(socket.socket, "connect", refuse)
    monkeypatch.setattr(socket, "create_connection", refuse)
    monkeypatch.setattr(socket, "getaddrinfo", refuse)
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", refuse)
    monkeypatch.setenv("PN2_NO_PRETRAINED", "1")
    monkeypatch.chdir(tmp_path)
    m = R.build("resnet50", pretrain=True)
    assert m.backbone.conv1.weight.shape == (64, 3, 7, 7)
    src = open(mirror.__file__).read()
    assert "http" not in src and "load_url" not in src and "model_zoo" not in src
    # a file that is there is loaded, from that path
    os.makedirs(tmp_path / "pretrained_pth" / "resnet")
    sd = mirror.resnet50().state_dict()
    sd["bn1.bias"] = sd["bn1.bias"] + 3.0
    torch.save(sd, tmp_path / "pretrained_pth" / "resnet" / "resnet50.pth")
    assert float(R.build("resnet50", pretrain=True).backbone.bn1.bias.detach().min()) == 3.0
    # without the switch a missing file is an error, as in the PVTv2 branch
    monkeypatch.setenv("PN2_NO_PRETRAINED", "0")
    with pytest.raises(FileNotFoundError):
        R.build("resnet101", pretrain=True)


def test_resnet50_single_supervision_stays_refused():
    """The one model two existing tests pin as refused (test_emcad_single_cpu.py, test_emcad_switches_cpu.py); its neighbours build."""
    with pytest.raises(NotImplementedError, match="single-supervision"):
        R.build("resnet50", dual=False)
    assert R.build("resnet152", dual=False).out_head4.in_channels == 2048 and R.build("resnet50", dual=True).dual


def test_basic_block_encoders_refused_by_name():
    from lib import resnet
    for enc in ("resnet18", "resnet34"):
        with pytest.raises(NotImplementedError, match="BasicBlock"):
            R.build(enc)
        assert not hasattr(resnet, enc)
    assert not hasattr(resnet, "BasicBlock")
    with pytest.raises(NotImplementedError):
        resnet.ResNet(resnet.Bottleneck, [1, 1, 1, 1], deep_base=True)


def test_subsample_entry_points_refuse_bad_arguments_before_any_launch():
    """-1 null pointer, -2 geometry, -3 dtype.  Every call fails its argument check, which comes before the first HIP call: this needs the library but no GPU (the
    pointers are never dereferenced)."""
    from pn2 import capi, F32, BF16
    lib = capi.load()
    p, nul, st = C.c_void_p(4096), C.c_void_p(0), C.c_void_p(0)

    def fwd(dt=BF16, x=p, ld_x=64, y=p, ld_y=64, N=2, H=8, W=8, Cc=64, stride=2):
        return lib.pn2_subsample_fwd(dt, x, ld_x, y, ld_y, N, H, W, Cc, stride, st)

    def bwd(dt=BF16, dy=p, ld_dy=64, dx=p, ld_dx=64, N=2, H=8, W=8, Cc=64, stride=2, accum=0):
        return lib.pn2_subsample_bwd(dt, dy, ld_dy, dx, ld_dx, N, H, W, Cc, stride, accum, st)
    for f in (fwd, bwd):
        a, b = ("x", "y") if f is fwd else ("dy", "dx")
        assert f(**{a: nul}) == -1 and f(**{b: nul}) == -1
        for dt in (2, 3, 7, -1):                                  # the conv-only codes (fp32fast, fp32x3) and unknown ones
            assert f(dt=dt) == -3, dt
        for s in (0, 3, -2, 4):
            assert f(stride=s) == -2, s
        for dt, bad in ((BF16, (4, 12, 68)), (F32, (2, 6, 66))):  # C off the 16-byte vector
            for c in bad:
                assert f(dt=dt, Cc=c, **{"ld_" + a: 128, "ld_" + b: 128}) == -2, (dt, c)
        assert f(dt=BF16, **{"ld_" + a: 68}) == -2 and f(dt=BF16, **{"ld_" + b: 68}) == -2          # ld off the vector
        assert f(dt=F32, **{"ld_" + a: 66}) == -2 and f(dt=F32, **{"ld_" + b: 66}) == -2
        assert f(**{"ld_" + a: 56}) == -2 and f(**{"ld_" + b: 56}) == -2                              # ld below C
        assert f(**{a: C.c_void_p(4096 + 8)}) == -2                                                  # rows off 16 bytes
        assert f(N=65536, H=65536, W=1) == -2 and f(N=3, H=32768, W=32768) == -2                     # N*H*W beyond 2^31 - 1
        assert f(N=0) == -2 and f(H=0) == -2 and f(W=-1) == -2 and f(Cc=0) == -2
    assert bwd(accum=2) == -2 and bwd(accum=-1) == -2
