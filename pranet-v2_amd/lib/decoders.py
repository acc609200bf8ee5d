"""EMCAD decoder, plain and with dual-supervised K-class heads (reference: multiclass_seg/EMCAD/lib/decoders.py) on the gfx950 kernels.

Same class names, constructor signatures and parameter names (state_dict keys) as the reference; the computation is expressed in
engine ops (pn2/engine.py + ops_*.py): 1x1 / 3x3 / 7x7 convs on the implicit-GEMM kernels, BatchNorm on pn2_bn_*, and the depth-wise, grouped,
gating, pooling, shuffle and up-sampling pieces on csrc/pn2_emcad.hip.  No PyTorch fallback: forward needs the GPU library.

The decoder switches of the reference's train_synapse.py (--kernel_sizes, --expansion_factor, --lgag_ks, --no_dw_parallel, --concatenation) are built
within these limits; anything else raises NotImplementedError (or the assert named below):
  kernel_sizes      1 to 4 sizes drawn from {1, 3, 5}, repeats allowed ([3,3,3], [5], [1,3,5,5]); a size of 7 or more, or a fifth branch, raises
  dw_parallel       True (every branch sees the same input) or False (sequential: branch i + 1 sees x + the outputs of branches 0..i)
  add               True: the branches are summed (three or fewer on pn2_gather_sum, four on pn2_msdc_combine); False: concatenated and shuffled in one
                    pass (pn2_msdc_combine, cat mode), pconv2 takes the n_scales * ex_channels wide input
  expansion_factor  any integer that keeps ex_channels a multiple of 8
  lgag_ks           3 (grouped 3x3 pair convs) or 1 (the reference then forces groups = 1: dense biased 1x1 convs on the pointwise conv path)
  activation        relu / relu6; leakyrelu, prelu, gelu and hswish raise
  MSCB              stride 1 and in_channels == out_channels stay asserted: EMCADNet builds nothing else
The default configuration ([1,3,5], expansion 2, parallel, add, lgag_ks 3, relu6) runs exactly the launches it ran before the switches were built.
"""
import math

import torch
import torch.nn as nn

from pn2 import F32
from pn2.graph import run_module


def gcd(a, b):
    while b:
        a, b = b, a % b
    return a


class BasicConv2d(nn.Module):
    """conv -> BN, no ReLU in forward (decoders.py:14-22)."""

    def __init__(self, in_planes, out_planes, kernel_size, stride=1, padding=0, dilation=1):
        super().__init__()
        self.conv = nn.Conv2d(in_planes, out_planes, kernel_size=kernel_size, stride=stride, padding=padding, dilation=dilation, bias=False)
        self.bn = nn.BatchNorm2d(out_planes)
        self.relu = nn.ReLU(inplace=True)

    def _build(self, eng, x):      # K-channel fp32 head map
        K = self.conv.out_channels
        return eng.conv_bn_act(x, self.conv, self.bn, out_map=(K, (K + 7) // 8 * 8), y_dt=F32, y_C=K)


def _init_weights(module, scheme='normal'):            # decoders.py:24-54 with the scheme every block passes
    for m in module.modules():
        if isinstance(m, nn.Conv2d):
            if scheme == 'normal':
                nn.init.normal_(m.weight, std=.02)
            else:
                fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels // m.groups
                nn.init.normal_(m.weight, 0, math.sqrt(2.0 / fan_out))
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, (nn.BatchNorm2d, nn.LayerNorm)):
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)


def act_layer(act, inplace=False):
    act = act.lower()
    if act == 'relu':
        return nn.ReLU(inplace)
    if act == 'relu6':
        return nn.ReLU6(inplace)
    raise NotImplementedError('activation layer [%s] is not built (relu / relu6 only)' % act)


def _act_code(m):
    return 2 if isinstance(m, nn.ReLU6) else True


class MSDC(nn.Module):
    """Multi-scale depth-wise convolutions (:83-102): k x k depth-wise conv + BN + act for every k, on the same input (dw_parallel) or each on the
    input plus the outputs of the branches before it (sequential, :117-126)."""
    MAX_BRANCHES, SIZES = 4, (1, 3, 5)

    def __init__(self, in_channels, kernel_sizes, stride, activation='relu6', dw_parallel=True):
        super().__init__()
        assert stride == 1, "only the stride-1 configuration is built"
        kernel_sizes = list(kernel_sizes)
        if not 1 <= len(kernel_sizes) <= self.MAX_BRANCHES:
            raise NotImplementedError('MSDC with %d branches is not built (1 to %d kernel sizes)' % (len(kernel_sizes), self.MAX_BRANCHES))
        for k in kernel_sizes:
            if k not in self.SIZES:
                raise NotImplementedError('depth-wise kernel size %r is not built: the depth-wise kernels stop at 5 x 5 (sizes 1, 3, 5)' % (k,))
        self.in_channels, self.kernel_sizes, self.activation, self.dw_parallel = in_channels, kernel_sizes, activation, dw_parallel
        self.dwconvs = nn.ModuleList([
            nn.Sequential(nn.Conv2d(in_channels, in_channels, k, stride, k // 2, groups=in_channels, bias=False), nn.BatchNorm2d(in_channels), act_layer(activation, inplace=True))
            for k in kernel_sizes])
        _init_weights(self)

    def _build(self, eng, x):
        if self.dw_parallel:
            return [eng.dwconv_bn_act(x, seq[0], seq[1], relu=_act_code(seq[2])) for seq in self.dwconvs]
        outs = []
        for i, seq in enumerate(self.dwconvs):
            outs.append(eng.dwconv_bn_act(x, seq[0], seq[1], relu=_act_code(seq[2])))
            if i + 1 < len(self.dwconvs):         # (the reference also forms the sum behind the last branch and drops it)
                x = eng.add(x, outs[-1])
        return outs


class MSCB(nn.Module):
    """Multi-scale convolution block (:104-164)."""

    def __init__(self, in_channels, out_channels, stride, kernel_sizes=[1, 3, 5], expansion_factor=2, dw_parallel=True, add=True, activation='relu6'):
        super().__init__()
        assert stride == 1 and in_channels == out_channels, "only the stride-1 / in == out configuration is built"
        self.in_channels, self.out_channels, self.stride, self.kernel_sizes = in_channels, out_channels, stride, kernel_sizes
        self.expansion_factor, self.dw_parallel, self.add, self.activation = expansion_factor, dw_parallel, add, activation
        self.n_scales = len(kernel_sizes)
        self.use_skip_connection = True
        self.ex_channels = int(in_channels * expansion_factor)
        if expansion_factor != int(expansion_factor) or self.ex_channels < 8 or self.ex_channels % 8:
            raise NotImplementedError('expansion_factor %r is not built: an integer that keeps ex_channels (%d) a multiple of 8' % (expansion_factor, self.ex_channels))
        self.pconv1 = nn.Sequential(nn.Conv2d(in_channels, self.ex_channels, 1, 1, 0, bias=False), nn.BatchNorm2d(self.ex_channels), act_layer(activation, inplace=True))
        self.msdc = MSDC(self.ex_channels, kernel_sizes, stride, activation, dw_parallel=dw_parallel)
        self.combined_channels = self.ex_channels if add else self.ex_channels * self.n_scales
        self.pconv2 = nn.Sequential(nn.Conv2d(self.combined_channels, out_channels, 1, 1, 0, bias=False), nn.BatchNorm2d(out_channels))
        _init_weights(self)

    def _build(self, eng, x):
        t = eng.conv_bn_act(x, self.pconv1[0], self.pconv1[1], relu=_act_code(self.pconv1[2]))
        parts, groups = self.msdc._build(eng, t), gcd(self.combined_channels, self.out_channels)
        if self.add:         # a sequential branch output has a second consumer (the next branch's input): no shared gradient tensor then
            dout = eng.shuffled_sum(parts, groups, shared_grad=self.dw_parallel or len(parts) == 1)
        else:
            dout = eng.shuffled_cat(parts, groups)
        return eng.conv_bn_act(dout, self.pconv2[0], self.pconv2[1], residual=x)


def MSCBLayer(in_channels, out_channels, n=1, stride=1, kernel_sizes=[1, 3, 5], expansion_factor=2, dw_parallel=True, add=True, activation='relu6'):
    convs = [MSCB(in_channels, out_channels, stride, kernel_sizes=kernel_sizes, expansion_factor=expansion_factor, dw_parallel=dw_parallel, add=add, activation=activation)]
    for _ in range(1, n):
        convs.append(MSCB(out_channels, out_channels, 1, kernel_sizes=kernel_sizes, expansion_factor=expansion_factor, dw_parallel=dw_parallel, add=add, activation=activation))
    return nn.Sequential(*convs)


class EUCB(nn.Module):
    """Efficient up-convolution block (:166-186): nearest x2, depth-wise 3x3 + BN + ReLU, channel_shuffle(groups = channels) = identity, biased 1x1."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, activation='relu'):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.up_dwc = nn.Sequential(nn.Upsample(scale_factor=2),
                                    nn.Conv2d(in_channels, in_channels, kernel_size=kernel_size, stride=stride, padding=kernel_size // 2, groups=in_channels, bias=False),
                                    nn.BatchNorm2d(in_channels), act_layer(activation, inplace=True))
        self.pwc = nn.Sequential(nn.Conv2d(in_channels, out_channels, kernel_size=1, stride=1, padding=0, bias=True))
        _init_weights(self)

    def _build(self, eng, x):
        t = eng.dwconv_bn_act(eng.upsample2x(x), self.up_dwc[1], self.up_dwc[2], relu=_act_code(self.up_dwc[3]))
        return eng.conv_bias(t, self.pwc[0])


class LGAG(nn.Module):
    """Large-kernel grouped attention gate (:188-214)."""

    def __init__(self, F_g, F_l, F_int, kernel_size=3, groups=1, activation='relu'):
        super().__init__()
        if kernel_size == 1:
            groups = 1
        if kernel_size not in (1, 3):
            raise NotImplementedError('LGAG kernel size %r is not built (1 or 3)' % (kernel_size,))
        assert F_g == F_l and activation == 'relu' and (kernel_size == 1 or (groups == F_int and F_g == 2 * F_int)), \
            "only the EMCAD configurations (3x3 with groups = F_int = C/2, or dense 1x1) are built"
        self.kernel_size = kernel_size
        self.W_g = nn.Sequential(nn.Conv2d(F_g, F_int, kernel_size=kernel_size, stride=1, padding=kernel_size // 2, groups=groups, bias=True), nn.BatchNorm2d(F_int))
        self.W_x = nn.Sequential(nn.Conv2d(F_l, F_int, kernel_size=kernel_size, stride=1, padding=kernel_size // 2, groups=groups, bias=True), nn.BatchNorm2d(F_int))
        self.psi = nn.Sequential(nn.Conv2d(F_int, 1, kernel_size=1, stride=1, padding=0, bias=True), nn.BatchNorm2d(1), nn.Sigmoid())
        self.activation = act_layer(activation, inplace=True)
        _init_weights(self)

    def _build(self, eng, g, x):
        if self.kernel_size == 1:           # dense biased 1x1 convs
            g1 = eng.conv_bn_act(g, self.W_g[0], self.W_g[1], bias=self.W_g[0].bias)
            t = eng.conv_bn_act(x, self.W_x[0], self.W_x[1], bias=self.W_x[0].bias, relu=True, residual=g1)
        else:
            g1 = eng.pairconv_bn(g, self.W_g[0], self.W_g[1])
            t = eng.pairconv_bn(x, self.W_x[0], self.W_x[1], relu=True, residual=g1)             # relu(g1 + x1)
        pre = eng.conv_bn_act(t, self.psi[0], self.psi[1], bias=self.psi[0].bias, out_map=(1, 8), y_dt=F32, y_C=1)
        return eng.sigmoid_gate(x, pre, 1)


class CAB(nn.Module):
    """Channel attention block (:216-241): returns the gated input (the reference returns the gate and multiplies at the call site)."""

    def __init__(self, in_channels, out_channels=None, ratio=16, activation='relu'):
        super().__init__()
        self.in_channels = in_channels
        if in_channels < ratio:
            ratio = in_channels
        self.reduced_channels = in_channels // ratio
        self.out_channels = in_channels if out_channels is None else out_channels
        assert self.out_channels == in_channels
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.max_pool = nn.AdaptiveMaxPool2d(1)
        self.activation = act_layer(activation, inplace=True)
        self.fc1 = nn.Conv2d(in_channels, self.reduced_channels, 1, bias=False)
        self.fc2 = nn.Conv2d(self.reduced_channels, self.out_channels, 1, bias=False)
        self.sigmoid = nn.Sigmoid()
        _init_weights(self)

    def _build_gated(self, eng, x):
        """cab(x) * x"""
        avg, mx = eng.global_pool(x)
        f = lambda t: eng.conv_bn_act(eng.conv_bn_act(t, self.fc1, None, relu=True), self.fc2, None)
        return eng.sigmoid_gate(x, eng.add(f(avg), f(mx)), 0)


class SAB(nn.Module):
    """Spatial attention block (:243-258)."""

    def __init__(self, kernel_size=7):
        super().__init__()
        assert kernel_size in (3, 7, 11), 'kernel must be 3 or 7 or 11'
        self.conv = nn.Conv2d(2, 1, kernel_size, padding=kernel_size // 2, bias=False)
        self.sigmoid = nn.Sigmoid()
        _init_weights(self)

    def _build_gated(self, eng, x):
        """sab(x) * x"""
        pre = eng.conv_bn_act(eng.chan_stats(x), self.conv, None, out_map=(1, 8), y_dt=F32, y_C=1)
        return eng.sigmoid_gate(x, pre, 1)


class _EMCADStages(nn.Module):
    """What EMCAD and EMCAD_dual share: the MSCAM stages (CAB, SAB, MSCB), the EUCB up-convolutions and the LGAG gates, registered in the reference's order
    (decoders.py:334-353 = :411-430), and the steps of their forward passes."""

    def _register_stages(self, channels, kernel_sizes, expansion_factor, dw_parallel, add, lgag_ks, activation):
        eucb_ks = 3
        mk = lambda c: MSCBLayer(c, c, n=1, stride=1, kernel_sizes=kernel_sizes, expansion_factor=expansion_factor, dw_parallel=dw_parallel, add=add, activation=activation)
        self.mscb4 = mk(channels[0])
        for i, lvl in ((1, 3), (2, 2), (3, 1)):
            setattr(self, f"eucb{lvl}", EUCB(in_channels=channels[i - 1], out_channels=channels[i], kernel_size=eucb_ks, stride=eucb_ks // 2))
            setattr(self, f"lgag{lvl}", LGAG(F_g=channels[i], F_l=channels[i], F_int=channels[i] // 2, kernel_size=lgag_ks, groups=channels[i] // 2))
            setattr(self, f"mscb{lvl}", mk(channels[i]))
        for i, lvl in enumerate((4, 3, 2, 1)):
            setattr(self, f"cab{lvl}", CAB(channels[i]))
        self.sab = SAB()

    def _stage(self, eng, d, lvl):
        """MSCAM: channel gate, spatial gate, multi-scale convolution block"""
        d = getattr(self, f"cab{lvl}")._build_gated(eng, d)
        d = self.sab._build_gated(eng, d)
        return getattr(self, f"mscb{lvl}")[0]._build(eng, d)

    def _gated_stage(self, eng, d, lvl, skip):
        """additive aggregation of the up-convolved map with its LGAG-gated skip, then the MSCAM stage"""
        d = eng.add(d, getattr(self, f"lgag{lvl}")._build(eng, d, skip))
        return self._stage(eng, d, lvl)


class EMCAD(_EMCADStages):
    """EMCAD decoder (:330-405): the four stage outputs; EMCADNet puts its out_head convs on them."""

    def __init__(self, channels=[512, 320, 128, 64], kernel_sizes=[1, 3, 5], expansion_factor=6, dw_parallel=True, add=True, lgag_ks=3, activation='relu6'):
        super().__init__()
        self._register_stages(channels, kernel_sizes, expansion_factor, dw_parallel, add, lgag_ks, activation)

    def _build(self, eng, x, skips):
        """forward :356-405 -> [d4, d3, d2, d1]"""
        d = self._stage(eng, x, 4)
        ds = [d]
        for lvl, skip in ((3, skips[0]), (2, skips[1]), (1, skips[2])):
            d = self._gated_stage(eng, getattr(self, f"eucb{lvl}")._build(eng, d), lvl, skip)
            ds.append(d)
        return ds


class EMCAD_dual(_EMCADStages):
    """EMCAD decoder with the dual-supervised reverse-attention heads (:407-526)."""

    def __init__(self, channels=[512, 320, 128, 64], kernel_sizes=[1, 3, 5], expansion_factor=6, dw_parallel=True, add=True, lgag_ks=3, activation='relu6', num_class=None):
        super().__init__()
        assert num_class is not None
        self._register_stages(channels, kernel_sizes, expansion_factor, dw_parallel, add, lgag_ks, activation)
        for i, lvl in enumerate((4, 3, 2, 1)):
            k, p = (1, 0) if lvl == 4 else (3, 1)
            setattr(self, f"ConvBlock{lvl}_fg", BasicConv2d(channels[i], num_class, kernel_size=k, padding=p))
            setattr(self, f"ConvBlock{lvl}_bg", BasicConv2d(channels[i], num_class, kernel_size=k, padding=p))

    def _build(self, eng, x, skips):
        """forward :441-526 -> [d4_fg, d3_fg, d2_fg, d1_fg, d4_bg, d3_bg, d2_bg, d1_bg] (low-resolution K-channel fp32 maps)"""
        d = self._stage(eng, x, 4)
        fg, bg = self.ConvBlock4_fg._build(eng, d), self.ConvBlock4_bg._build(eng, d)
        fgs, bgs = [fg], [bg]
        for lvl, skip in ((3, skips[0]), (2, skips[1]), (1, skips[2])):
            d = getattr(self, f"eucb{lvl}")._build(eng, d)
            up_fg, up_bg = eng.resize_to(fg, d.H, d.W), eng.resize_to(bg, d.H, d.W)
            d = self._gated_stage(eng, d, lvl, skip)
            fg, bg = getattr(self, f"ConvBlock{lvl}_fg")._build(eng, d), getattr(self, f"ConvBlock{lvl}_bg")._build(eng, d)
            fg = eng.dsra_fuse(fg, up_fg, up_bg, True)
            fgs.append(fg); bgs.append(bg)
        return fgs + bgs
