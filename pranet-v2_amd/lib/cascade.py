"""CASCADE decoders - concatenating, additive and dual-supervised (reference: multiclass_seg/MIST/lib/decoders.py:20-431; MERIT's copy is the same text) on the gfx950 kernels.

Same class names, constructor signatures, parameter names (state_dict keys and order) and default initialisation as the reference; the computation is expressed in
engine ops, as in lib/decoders.py: the biased 3x3 / 1x1 convs on the implicit-GEMM kernels with BatchNorm on pn2_bn_*, nearest x2 up-sampling, the channel and
spatial attention of the CAM blocks on the pooling and gating kernels of csrc/pn2_emcad.hip, the DSRA fusion on pn2_dsra_fuse, and the attention gate together with
the aggregation behind it on csrc/pn2_cascade.hip: g + x * psi (Engine.attention_gate) or cat(x * psi, g) (Engine.attention_gate_cat), each written by one launch.
No PyTorch fallback: forward needs the GPU library.

Built: CASCADE_Cat, CASCADE_Add and CASCADE_Add_dual (both use_softmax values).  The reference's ChannelAttention divides its width by 16 whatever the width, so a stage
needs at least 16 channels there; the same holds here.  CASCADE_Cat's gated stages need widths that are a multiple of 8 (every reference width is): the two halves of a
concatenated row then both start on a 16-byte boundary."""
import torch
import torch.nn as nn

from pn2 import F32
from pn2.graph import run_module
from lib.decoders import BasicConv2d


class conv_block(nn.Module):
    """(3x3 conv + bias -> BN -> ReLU) twice (:20-35)."""

    def __init__(self, ch_in, ch_out):
        super().__init__()
        self.conv = nn.Sequential(
            nn.Conv2d(ch_in, ch_out, kernel_size=3, stride=1, padding=1, bias=True), nn.BatchNorm2d(ch_out), nn.ReLU(inplace=True),
            nn.Conv2d(ch_out, ch_out, kernel_size=3, stride=1, padding=1, bias=True), nn.BatchNorm2d(ch_out), nn.ReLU(inplace=True))

    def _build(self, eng, x):
        t = eng.conv_bn_act(x, self.conv[0], self.conv[1], relu=True, bias=self.conv[0].bias)
        return eng.conv_bn_act(t, self.conv[3], self.conv[4], relu=True, bias=self.conv[3].bias)

    def forward(self, x):
        return run_module(lambda eng, a: [self._build(eng, a)], [x], list(self.parameters()), self.training)[0]


class up_conv(nn.Module):
    """nearest x2 -> 3x3 conv + bias -> BN -> ReLU (:37-49)."""

    def __init__(self, ch_in, ch_out, kernel_size=3, stride=1, padding=1, groups=1):
        super().__init__()
        self.up = nn.Sequential(nn.Upsample(scale_factor=2), nn.Conv2d(ch_in, ch_out, kernel_size=kernel_size, stride=stride, padding=padding, bias=True),
                                nn.BatchNorm2d(ch_out), nn.ReLU(inplace=True))

    def _build(self, eng, x):
        return eng.conv_bn_act(eng.upsample2x(x), self.up[1], self.up[2], relu=True, bias=self.up[1].bias)

    def forward(self, x):
        return run_module(lambda eng, a: [self._build(eng, a)], [x], list(self.parameters()), self.training)[0]


class Attention_block(nn.Module):
    """Additive attention gate (:52-79).  _build_aggregate returns g + x * psi, _build_concat cat(x * psi, g): the gate and the "aggregate" / "Concat" line that follows
    every one of its uses, in one op."""

    def __init__(self, F_g, F_l, F_int):
        super().__init__()
        self.W_g = nn.Sequential(nn.Conv2d(F_g, F_int, kernel_size=1, stride=1, padding=0, bias=True), nn.BatchNorm2d(F_int))
        self.W_x = nn.Sequential(nn.Conv2d(F_l, F_int, kernel_size=1, stride=1, padding=0, bias=True), nn.BatchNorm2d(F_int))
        self.psi = nn.Sequential(nn.Conv2d(F_int, 1, kernel_size=1, stride=1, padding=0, bias=True), nn.BatchNorm2d(1), nn.Sigmoid())
        self.relu = nn.ReLU(inplace=True)

    def _check(self, g, x):
        if g.C != x.C:
            raise NotImplementedError("Attention_block with F_g != F_l is not built: the fused gate adds x * psi to g (every CASCADE decoder uses one width)")
        if self.psi[0].in_channels > 256:
            raise NotImplementedError("Attention_block with F_int above 256 is not built (the gate kernels take at most 64 fp32 channel vectors)")

    def _build_aggregate(self, eng, g, x):
        self._check(g, x)
        return eng.attention_gate(g, x, self.W_g[0], self.W_g[1], self.W_x[0], self.W_x[1], self.psi[0], self.psi[1])

    def _build_concat(self, eng, g, x):
        self._check(g, x)
        if g.C % 8:
            raise NotImplementedError(f"Attention_block behind a concatenation needs a width that is a multiple of 8, not {g.C} (the halves of a row are 16-byte vectors)")
        return eng.attention_gate_cat(g, x, self.W_g[0], self.W_g[1], self.W_x[0], self.W_x[1], self.psi[0], self.psi[1])

    def forward(self, g, x):
        """x * psi, as the reference returns it: the fused op's g + x * psi minus g"""
        return run_module(lambda eng, a, b: [self._build_aggregate(eng, a, b)], [g, x], list(self.parameters()), self.training)[0] - g


class ChannelAttention(nn.Module):
    """(:81-102); returns the gated input (the reference returns the gate and multiplies at the call site)."""

    def __init__(self, in_planes, ratio=16):
        super().__init__()
        self.in_planes = in_planes
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.max_pool = nn.AdaptiveMaxPool2d(1)
        self.fc1 = nn.Conv2d(in_planes, in_planes // 16, 1, bias=False)
        self.relu1 = nn.ReLU()
        self.fc2 = nn.Conv2d(in_planes // 16, in_planes, 1, bias=False)
        self.sigmoid = nn.Sigmoid()

    def _build_pre(self, eng, x):
        if self.in_planes < 16:
            raise NotImplementedError("ChannelAttention below 16 channels has an empty bottleneck (in_planes // 16 = 0)")
        avg, mx = eng.global_pool(x)
        f = lambda t: eng.conv_bn_act(eng.conv_bn_act(t, self.fc1, None, relu=True), self.fc2, None)
        return eng.add(f(avg), f(mx))

    def _build_gated(self, eng, x):
        return eng.sigmoid_gate(x, self._build_pre(eng, x), 0)

    def forward(self, x):
        """the gate [N, C, 1, 1], as the reference returns it"""
        return torch.sigmoid(run_module(lambda eng, a: [self._build_pre(eng, a)], [x], list(self.parameters()), self.training)[0])


class SpatialAttention(nn.Module):
    """(:104-119); returns the gated input."""

    def __init__(self, kernel_size=7):
        super().__init__()
        assert kernel_size in (3, 7), 'kernel size must be 3 or 7'
        padding = 3 if kernel_size == 7 else 1
        self.conv1 = nn.Conv2d(2, 1, kernel_size, padding=padding, bias=False)
        self.sigmoid = nn.Sigmoid()

    def _build_pre(self, eng, x):
        return eng.conv_bn_act(eng.chan_stats(x), self.conv1, None, out_map=(1, 8), y_dt=F32, y_C=1)

    def _build_gated(self, eng, x):
        return eng.sigmoid_gate(x, self._build_pre(eng, x), 1)

    def forward(self, x):
        """the gate [N, 1, H, W], as the reference returns it"""
        return torch.sigmoid(run_module(lambda eng, a: [self._build_pre(eng, a)], [x], list(self.parameters()), self.training)[0])


class _CascadeStages(nn.Module):
    """What the CASCADE decoders share; with a `num_class` the dual-supervised fg / bg heads are registered in the reference's order (behind each stage's ConvBlock).
    `width`: how many times the stage width the CAM of a gated stage is wide (2: the gate's output is concatenated with the up-sampled map, CASCADE_Cat)."""

    def _register_stages(self, channels, num_class=None, width=1):
        c = channels
        self.Conv_1x1 = nn.Conv2d(c[0], c[0], kernel_size=1, stride=1, padding=0)
        self.ConvBlock4 = conv_block(ch_in=c[0], ch_out=c[0])
        self._register_heads(4, c[0], num_class)
        for i, lvl in ((1, 3), (2, 2), (3, 1)):
            setattr(self, f"Up{lvl}", up_conv(ch_in=c[i - 1], ch_out=c[i]))
            setattr(self, f"AG{lvl}", Attention_block(F_g=c[i], F_l=c[i], F_int=c[i + 1] if lvl > 1 else int(c[3] / 2)))
            setattr(self, f"ConvBlock{lvl}", conv_block(ch_in=width * c[i], ch_out=c[i]))
            self._register_heads(lvl, c[i], num_class)
        for i, lvl in enumerate((4, 3, 2, 1)):
            setattr(self, f"CA{lvl}", ChannelAttention(c[i] if lvl == 4 else width * c[i]))
        self.SA = SpatialAttention()

    def _register_heads(self, lvl, ch, num_class):
        if num_class is not None:
            k, p = (1, 0) if lvl == 4 else (3, 1)
            setattr(self, f"ConvBlock{lvl}_fg", BasicConv2d(ch, num_class, kernel_size=k, padding=p))
            setattr(self, f"ConvBlock{lvl}_bg", BasicConv2d(ch, num_class, kernel_size=k, padding=p))

    def _cam(self, eng, d, lvl):
        """CAM: channel gate, spatial gate, conv block"""
        d = getattr(self, f"CA{lvl}")._build_gated(eng, d)
        d = self.SA._build_gated(eng, d)
        return getattr(self, f"ConvBlock{lvl}")._build(eng, d)

    def _gated_cam(self, eng, d, lvl, skip, concat=False):
        ag = getattr(self, f"AG{lvl}")
        return self._cam(eng, ag._build_concat(eng, d, skip) if concat else ag._build_aggregate(eng, d, skip), lvl)

    def _build_stages(self, eng, x, skips, concat):
        """the four CAM stages without heads -> [d4, d3, d2, d1]"""
        d = self._cam(eng, eng.conv_bias(x, self.Conv_1x1), 4)
        ds = [d]
        for lvl, skip in ((3, skips[0]), (2, skips[1]), (1, skips[2])):
            d = self._gated_cam(eng, getattr(self, f"Up{lvl}")._build(eng, d), lvl, skip, concat)
            ds.append(d)
        return ds

    def _params(self):
        return list(self.parameters())

    def forward(self, x, skips):
        return run_module(lambda eng, x_, *s: self._build(eng, x_, list(s)), [x, *skips], self._params(), self.training)


class CASCADE_Cat(_CascadeStages):
    """CASCADE decoder with concatenating aggregation (:121-199): (d4, d3, d2, d1).  cat(AG(g, x), g) feeds a CAM of twice the stage width."""

    def __init__(self, channels=[512, 320, 128, 64]):
        super().__init__()
        self._register_stages(channels, width=2)

    def _build(self, eng, x, skips):
        return self._build_stages(eng, x, skips, True)


class CASCADE_Add(_CascadeStages):
    """CASCADE decoder with additive aggregation (:202-286): (d4, d3, d2, d1)."""

    def __init__(self, channels=[512, 320, 128, 64]):
        super().__init__()
        self._register_stages(channels)

    def _build(self, eng, x, skips):
        return self._build_stages(eng, x, skips, False)


class CASCADE_Add_dual(_CascadeStages):
    """CASCADE decoder with the dual-supervised reverse-attention heads (:289-431): (d4_fg, d3_fg, d2_fg, d1_fg, d4_bg, d3_bg, d2_bg, d1_bg, d1)."""

    def __init__(self, channels=[512, 320, 128, 64], num_class=None, use_softmax=True):
        super().__init__()
        assert num_class is not None
        self.use_softmax = use_softmax
        self._register_stages(channels, num_class)

    def _build(self, eng, x, skips):
        d = self._cam(eng, eng.conv_bias(x, self.Conv_1x1), 4)
        fg, bg = self.ConvBlock4_fg._build(eng, d), self.ConvBlock4_bg._build(eng, d)
        fgs, bgs = [fg], [bg]
        for lvl, skip in ((3, skips[0]), (2, skips[1]), (1, skips[2])):
            d = getattr(self, f"Up{lvl}")._build(eng, d)
            up_fg, up_bg = eng.resize_to(fg, d.H, d.W), eng.resize_to(bg, d.H, d.W)
            d = self._gated_cam(eng, d, lvl, skip)
            fg, bg = getattr(self, f"ConvBlock{lvl}_fg")._build(eng, d), getattr(self, f"ConvBlock{lvl}_bg")._build(eng, d)
            fg = eng.dsra_fuse(fg, up_fg, up_bg, self.use_softmax)
            fgs.append(fg); bgs.append(bg)
        return fgs + bgs + [d]
