"""Engine ops, part 5: the strided skip of the ResNet stage-opening blocks (csrc/pn2_resnet.hip).  Mixed into pn2.engine.Engine."""
from .capi import call, F32
from .core import Act, _p, _stream


class _Stride1View:
    """The 1x1 conv `conv` (stride s, pad 0) as the stride-1 conv it is on rows that were gathered with stride s: the SAME weight parameter (no copy - the packed
    panels are keyed by it and its gradient lands in its own sink), other geometry."""
    __slots__ = ("weight", "stride", "padding", "dilation", "groups")

    def __init__(self, conv):
        self.weight, self.stride, self.padding, self.dilation, self.groups = conv.weight, (1, 1), (0, 0), (1, 1), 1


class ResNetOps:
    def subsample(self, x, stride):
        """x[:, ::stride, ::stride, :] as a new activation (pn2_subsample_fwd); the backward scatters into the WHOLE of x's gradient in one pass (pn2_subsample_bwd): as the
        first contribution it writes the zeros between the strided pixels itself, as a later one it adds to the strided pixels only.  stride 1: x itself."""
        if stride == 1:
            return x
        V = 4 if x.dt == F32 else 8
        if stride != 2 or x.Cp % V or x.ld % V:
            raise NotImplementedError(f"subsample: stride {stride}, {x.Cp} channels in rows of {x.ld} - stride 2 on 16-byte aligned rows is built")
        N, H, W = x.N, x.H, x.W
        OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
        y = Act(self, self.empty(N, OH, OW, x.Cp, x.dt), x.C, x.gw, x.gwp, x.dt, requires_grad=x.requires_grad)
        call.pn2_subsample_fwd(x.dt, x.ptr, x.ld, y.ptr, y.ld, N, H, W, x.Cp, stride, _stream())

        def bwd():
            if not x.requires_grad:
                return
            gy = y.grad_buf()
            gx, acc = x.grad_sink()
            call.pn2_subsample_bwd(x.dt, _p(gy), gy.stride(2), _p(gx), gx.stride(2), N, H, W, x.Cp, stride, acc, _stream())
        self.record(bwd)
        return y

    def strided_pointwise(self, x, conv, bn, **kw):
        """conv_bn_act of a bias-free 1x1 conv with stride 2 and no padding (the downsample branch of a ResNet stage-opening block, EMCAD/lib/resnet.py:141-148) as
        subsample + the stride-1 pointwise conv path on the rows that are left: the GEMM, its BatchNorm statistics, the weight gradient and the data gradient all run on
        a quarter of the pixels, on the launches every other 1x1 conv takes.  kw goes to conv_bn_act (defer_out=True: the BatchNorm output folds into the residual
        consumer's pass, as in Bottle2neck)."""
        (sh, sw), w = conv.stride, conv.weight
        if tuple(w.shape[2:]) != (1, 1) or sh != sw or tuple(conv.padding) != (0, 0) or conv.groups != 1 or conv.bias is not None:
            raise NotImplementedError("strided_pointwise: a bias-free dense 1x1 conv without padding")
        if sh == 1:
            return self.conv_bn_act(x, conv, bn, **kw)
        return self.conv_bn_act(self.subsample(x, sh), _Stride1View(conv), bn, **kw)
