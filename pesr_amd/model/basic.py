"""Building blocks with the reference's constructors and state_dict schema (reference model/basic.py),
running on the HIP kernels of libpesr_hip.so.

Every module takes and returns logical NCHW fp32 tensors; outputs are in torch.channels_last memory
format (NHWC physically), so chaining modules never copies.  CPU tensors raise: there is no fallback.
Parameters keep the reference's names, shapes (OIHW) and default initialisation (drawn through the very
torch initialisers the reference's nn.Conv2d / nn.Linear would call, in the same order, so a seeded
construction consumes the RNG identically).
"""
import torch
import torch.nn as nn

from .. import functional as PF
from .. import ops


def nhwc(x: torch.Tensor) -> torch.Tensor:
    """logical NCHW -> NHWC view (zero-copy for channels_last inputs)."""
    return x.permute(0, 2, 3, 1)


def nchw(y: torch.Tensor) -> torch.Tensor:
    """NHWC tensor -> logical NCHW view (channels_last strides)."""
    return y.permute(0, 3, 1, 2)


def spectral_norm(conv, eps=1e-12):
    """reference model/basic.py:25 calls `spectral_norm(Conv(...))` without importing it (NameError when --spectral_norm true,
    SURVEY Q3); the evident intent - torch.nn.utils.spectral_norm, one power iteration per training forward - is what this
    does to a pesr_amd Conv: same parameter / buffer names (`weight_orig`, `weight_u`, `weight_v`: torch's state_dict schema),
    same RNG draws in the same order (u then v, standard normal, normalised), the normalised weight computed by the HIP
    kernels of spectral_norm.hip at every forward."""
    import torch.nn.functional as F
    w = conv.weight
    with torch.no_grad():
        u = F.normalize(w.new_empty(w.shape[0]).normal_(0, 1), dim=0, eps=eps)
        v = F.normalize(w.new_empty(w[0].numel()).normal_(0, 1), dim=0, eps=eps)
    del conv.weight
    conv.register_parameter("weight_orig", w)
    conv.register_buffer("weight_u", u)
    conv.register_buffer("weight_v", v)
    conv._sn_eps = eps
    return conv


class Conv(nn.Module):
    """k x k conv, padding k//2 (reference model/basic.py:4-7).  kernel_size 3 - the only size the reference's networks use -
    runs on the MFMA / Winograd kernels; any other odd size on the generic kernels of conv_kxk.hip (complete, untuned)."""

    def __init__(self, in_planes, out_planes, kernel_size, stride=1, bias=True):
        super().__init__()
        if kernel_size % 2 == 0:
            raise NotImplementedError("pesr_amd Conv: even kernel sizes change the output size under padding k//2; odd sizes only")
        init = nn.Conv2d(in_planes, out_planes, kernel_size, padding=kernel_size // 2, stride=stride, bias=bias)
        self.weight = nn.Parameter(init.weight.data)
        self.bias = nn.Parameter(init.bias.data) if bias else None
        self.in_channels, self.out_channels, self.stride, self.kernel_size = in_planes, out_planes, stride, kernel_size
        self.packed = PF.PackedConvWeights(ps=False)
        self._sn_eps = None          # set by spectral_norm(): the weight is then weight_orig / sigma, recomputed per forward

    def effective_weight(self):
        """The weight this forward convolves with: the parameter itself, or - under spectral_norm - weight_orig / sigma."""
        if self._sn_eps is None:
            return self.weight
        return PF.spectral_normalize(self.weight_orig, self.weight_u, self.weight_v, self.training, self._sn_eps)

    def forward(self, x, act=ops.ACT_NONE, relu_in=False, relu_grad_by_consumer=False, precision=None):
        """precision: None, or the mode this call's forward AND backward run under whatever ops.PRECISION is then (3 x 3 only)."""
        if self.kernel_size != 3:
            assert act == ops.ACT_NONE and not relu_in and precision is None, "fused activations exist for the 3x3 kernels only"
            return nchw(PF.ConvKxKFn.apply(nhwc(x), self.effective_weight(), self.bias, self.stride))
        return nchw(PF.conv3x3(nhwc(x), self.effective_weight(), self.bias, self.packed, self.stride, act, relu_in,
                               relu_grad_by_consumer, precision))

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, "
                f"bias={self.bias is not None}")


class MeanShift(nn.Module):
    """1x1 conv 3->3 initialised to (x -/+ rgb_range*mean)/std (reference model/basic.py:9-17).  As in the
    reference, `self.requires_grad = False` is a no-op: weight and bias ARE trainable."""

    def __init__(self, rgb_range, rgb_mean, rgb_std, sign=-1):
        super().__init__()
        init = nn.Conv2d(3, 3, kernel_size=1)  # draws (then discards) an init, as the reference does
        std = torch.Tensor(rgb_std)
        w = torch.eye(3).view(3, 3, 1, 1)
        w.div_(std.view(3, 1, 1, 1))
        b = sign * rgb_range * torch.Tensor(rgb_mean)
        b.div_(std)
        self.weight = nn.Parameter(init.weight.data.copy_(w))
        self.bias = nn.Parameter(init.bias.data.copy_(b))
        self.requires_grad = False

    def forward(self, x):
        if x.dim() == 4 and x.is_contiguous() and not x.is_contiguous(memory_format=torch.channels_last):
            # NCHW-contiguous network input: the layout change is folded into the kernel
            return nchw(PF.MeanShiftFn.apply(x, self.weight, self.bias, True, False))
        return nchw(PF.MeanShiftFn.apply(nhwc(x), self.weight, self.bias, False, False))


class PixelShuffle(nn.Module):
    """nn.PixelShuffle(r), r = 2 or 3, as a standalone kernel (the x4 / x2 Upsampler fuses r = 2 into the conv epilogue
    instead; the x3 Upsampler runs this module's r = 3 kernel)."""

    def __init__(self, upscale_factor=2):
        super().__init__()
        if upscale_factor not in (2, 3):
            raise ValueError(f"PixelShuffle: upscale_factor {upscale_factor}; the HIP kernels implement 2 and 3")
        self.upscale_factor = upscale_factor

    def forward(self, x):
        if self.upscale_factor == 2:
            return nchw(_PixelShuffleFn.apply(nhwc(x)))
        return nchw(_PixelShuffleRFn.apply(nhwc(x), self.upscale_factor))


class _PixelShuffleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return ops.pixel_shuffle_fwd(x.contiguous())

    @staticmethod
    def backward(ctx, gy):
        return ops.pixel_shuffle_bwd(gy.contiguous())


class _PixelShuffleRFn(torch.autograd.Function):
    """NHWC [N,H,W,r*r*C] -> [N,r*H,r*W,C] on pixel_shuffle_r.hip; the backward is the same kernel's inverse."""

    @staticmethod
    def forward(ctx, x, r):
        ctx.r = r
        return ops.pixel_shuffle_r_fwd(x.contiguous(), r)

    @staticmethod
    def backward(ctx, gy):
        return ops.pixel_shuffle_r_bwd(gy.contiguous(), ctx.r), None


def _act_slope(act):
    """negative slope that stands for an activation module in the fused BN / conv epilogues (None: identity)."""
    if act is None:
        return 1.0
    if isinstance(act, nn.LeakyReLU):
        return float(act.negative_slope)
    if isinstance(act, nn.ReLU):
        return 0.0
    raise NotImplementedError(f"activation {type(act).__name__}: the HIP epilogues implement ReLU, LeakyReLU and none")


def _conv_act(conv, x_nhwc, act):
    """conv (+bias) followed by an activation module (or None), un-fused with whatever comes next."""
    slope = _act_slope(act)
    w = conv.effective_weight()
    if conv.kernel_size != 3:       # generic kernel, activation as its own (differentiable) elementwise op
        z = PF.ConvKxKFn.apply(x_nhwc, w, conv.bias, conv.stride)
        return z if slope == 1.0 else PF.LRelu2Fn.apply(z, slope)
    if slope == 1.0:
        return PF.conv3x3(x_nhwc, w, conv.bias, conv.packed, conv.stride)
    if slope == 0.0:
        return PF.conv3x3(x_nhwc, w, conv.bias, conv.packed, conv.stride, act=ops.ACT_RELU)
    return PF.ConvLReluFn.apply(x_nhwc, w, conv.bias, conv.packed, conv.stride, slope)


def _conv_bn_act(conv, bn, x_nhwc, act, y_nchw=False, prev_link=None, link=None):
    if conv.kernel_size != 3:       # generic conv -> BatchNorm -> activation, un-fused (training-mode statistics only)
        if not (bn.training or bn.running_mean is None):
            raise NotImplementedError("eval-mode BatchNorm behind a conv with kernel_size != 3")
        z = PF.ConvKxKFn.apply(x_nhwc, conv.effective_weight(), conv.bias, conv.stride)
        u = PF.Bn2Fn.apply(z, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.eps, bn.momentum)
        slope = _act_slope(act)
        y = u if slope == 1.0 else PF.LRelu2Fn.apply(u, slope)
        return nchw(y).contiguous() if y_nchw else y
    return PF.ConvBnLReluFn.apply(x_nhwc, conv.effective_weight(), conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                  bn.num_batches_tracked, conv.packed, conv.stride, bn.eps, bn.momentum, _act_slope(act), y_nchw,
                                  bn.training or bn.running_mean is None, prev_link, link)


class BasicBlock(nn.Sequential):
    """conv -> [BatchNorm2d] -> [act] (reference model/basic.py:19-31); the Discriminator's unit (no bias, BN in training mode,
    LeakyReLU(0.2)).  Every combination the constructor accepts runs on the HIP kernels: conv bias, bn on / off, BatchNorm in
    training or eval mode, act = ReLU / LeakyReLU / None."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, bias=False, bn=True, act=nn.ReLU(True),
                 sn=True):
        if sn:
            conv = spectral_norm(Conv(in_channels, out_channels, kernel_size, stride, bias))
        else:
            conv = Conv(in_channels, out_channels, kernel_size, stride, bias)
        m = [conv]
        if bn:
            m.append(nn.BatchNorm2d(out_channels))
        if act is not None:
            m.append(act)
        super().__init__(*m)
        self._has_bn, self._has_act = bn, act is not None
        self.flatten_output = False  # set by Discriminator on its last block: emit NCHW-contiguous for .view(B, -1)

    def forward_linked(self, x, prev_link):
        """forward() for a caller that chains blocks itself and keeps the tensors in between to itself (Discriminator.forward):
        -> (output, BnLink | None).  prev_link: the link returned for the block that produced x.  With the links the backward pass
        folds each block's BatchNorm reductions into the input-gradient kernel of the block behind it (functional.BnLink)."""
        conv = self[0]
        if not (self._has_bn and conv.kernel_size == 3 and self._has_act) or (self._has_bn and self[1].momentum is None):
            return self.forward(x), None
        link = None if self.flatten_output else PF.BnLink()
        y = _conv_bn_act(conv, self[1], nhwc(x), self[-1], self.flatten_output, prev_link, link)
        return (y if self.flatten_output else nchw(y)), link

    def forward(self, x):
        conv = self[0]
        bn = self[1] if self._has_bn else None
        act = self[-1] if self._has_act else None
        if bn is not None:
            y = _conv_bn_act(conv, bn, nhwc(x), act, self.flatten_output)
            return y if self.flatten_output else nchw(y)
        y = _conv_act(conv, nhwc(x), act)
        if self.flatten_output:
            return nchw(y).contiguous()
        return nchw(y)


ATTENTIONS = (None, "ca")


class ChannelAttention(nn.Module):
    """RCAN's squeeze-and-excite gate (Zhang et al., ECCV 2018) as the tail of a residual block (an extension, docs/modes.md section
    4u): forward(x, t, res_scale) = x + res_scale * t * sigmoid(excite(relu(squeeze(mean over the pixels of t)))).  squeeze and excite
    are 1 x 1 convs n_feats -> n_feats / reduction -> n_feats, initialised like nn.Conv2d, squeeze first; on a pooled [N, C, 1, 1] map
    they are two small matrix products, which the gate kernels do themselves (the Conv modules hold the parameters)."""

    def __init__(self, n_feats, reduction=16):
        super().__init__()
        hidden = ops.ca_check_channels("ChannelAttention", n_feats, reduction)
        self.squeeze = Conv(n_feats, hidden, 1)
        self.excite = Conv(hidden, n_feats, 1)
        self.n_feats, self.reduction = n_feats, reduction

    def forward(self, x_nhwc, t_nhwc, res_scale):
        return PF.ChannelAttentionFn.apply(x_nhwc, t_nhwc, self.squeeze.weight, self.squeeze.bias, self.excite.weight, self.excite.bias,
                                           float(res_scale))

    def extra_repr(self):
        return f"{self.n_feats}, reduction={self.reduction}"


class ChannelLayerNorm(nn.Module):
    """LayerNorm over the channels of each pixel (an extension, docs/modes.md section 4x): per pixel of an NHWC map, y = (x - mean) /
    sqrt(var + 1e-5) * weight + bias with the centred variance.  weight = 1, bias = 0: construction draws nothing from the RNG."""

    def __init__(self, n_feats):
        super().__init__()
        ops.ln_check_channels("ChannelLayerNorm", n_feats)
        self.weight = nn.Parameter(torch.ones(n_feats))
        self.bias = nn.Parameter(torch.zeros(n_feats))
        self.n_feats = n_feats

    def forward_nhwc(self, h):
        return PF.LayerNormFn.apply(h, self.weight, self.bias)

    def forward(self, x):
        return nchw(self.forward_nhwc(nhwc(x)))

    def extra_repr(self):
        return f"{self.n_feats}"


class WindowAttention(nn.Module):
    """A window self-attention block (an extension, docs/modes.md section 4w; the Swin / SwinIR form with conv projections as in CvT):
    forward(x) = x + proj(attention(qkv(x))).  qkv = Conv(n_feats, 3 dim, 3) gives q | k | v with heads of 32 channels, the attention
    runs inside 8 x 8 windows of a grid whose origin is (-shift, -shift) over the pixels inside the image, proj = Conv(dim, n_feats, 3)
    carries the skip addition in its epilogue.  The two convs are constructed in that order and initialised like every Conv; they run
    on the routed 3 x 3 kernels (and follow --precision), the attention itself is fp32.
    norm="ln" (section 4x) puts a ChannelLayerNorm in front of qkv, the pre-norm of every Swin layer: forward(x) = x +
    proj(attention(qkv(LN(x)))), the skip taking the un-normalised x.  It is registered after the two convs (their initial values and
    keys are those of the block without it).  norm=None: no such module, what the block was."""

    def __init__(self, n_feats, dim, shift=0, norm=None):
        super().__init__()
        ops.wattn_check_widths("WindowAttention", n_feats, dim)
        if shift not in range(ops.WATTN_WINDOW):
            raise ValueError(f"WindowAttention: shift = {shift!r}; expected 0 .. {ops.WATTN_WINDOW - 1}")
        if norm not in (None, "ln"):
            raise ValueError(f"WindowAttention: norm = {norm!r}; expected None or 'ln'")
        self.qkv = Conv(n_feats, 3 * dim, 3)
        self.proj = Conv(dim, n_feats, 3)
        if norm == "ln":
            self.norm = ChannelLayerNorm(n_feats)
        self.n_feats, self.dim, self.shift = n_feats, dim, shift

    def forward(self, x):
        h = nhwc(x)
        norm = getattr(self, "norm", None)
        u = PF.conv3x3(h if norm is None else norm.forward_nhwc(h), self.qkv.weight, self.qkv.bias, self.qkv.packed)
        o = PF.WindowAttentionFn.apply(u, self.shift)
        return nchw(PF.ConvAddFn.apply(o, h, self.proj.weight, self.proj.bias, self.proj.packed))

    def extra_repr(self):
        return f"{self.n_feats}, dim={self.dim}, shift={self.shift}" + (", norm=ln" if hasattr(self, "norm") else "")


class ResBlock(nn.Module):
    """x + res_scale * conv(act(conv(x))) (reference model/basic.py:33-52).  The reference's only configuration (bias, no BN,
    ReLU) is one fused autograd node; the other constructor branches (bn=True, bias=False, LeakyReLU) run un-fused on the
    same kernels.  attention="ca" (an extension): x + res_scale * t * gate(t) with t = conv(act(conv(x))), the gate a
    ChannelAttention(n_feats, reduction) constructed and registered after the two convs."""

    def __init__(self, n_feats, kernel_size, bias=True, bn=False, act=nn.ReLU(True), res_scale=1, attention=None, reduction=16):
        super().__init__()
        if attention not in ATTENTIONS:
            raise ValueError(f"ResBlock: attention = {attention!r}; supported are {ATTENTIONS}")
        _act_slope(act)       # rejects activations the epilogues do not implement
        modules_body = []
        for i in range(2):
            modules_body.append(Conv(n_feats, n_feats, kernel_size, bias=bias))
            if bn:
                modules_body.append(nn.BatchNorm2d(n_feats))
            if i == 0:
                modules_body.append(act)
        self.body = nn.Sequential(*modules_body)
        self.res_scale = res_scale
        self._bn = bn
        # the fused node runs the 3x3 kernels only: any other (odd) kernel size takes the un-fused path, whose _conv_act
        # routes it to the generic kernels (a [C,C,5,5] weight read by a 3x3 packer would be silently wrong)
        self._fused = kernel_size == 3 and bias and not bn and isinstance(act, nn.ReLU) and not isinstance(act, nn.LeakyReLU)
        if attention is not None:
            self.ca = ChannelAttention(n_feats, reduction)

    def forward(self, x):
        if hasattr(self, "ca"):
            return self._forward_attention(x)
        if self._fused:
            c1, c2 = self.body[0], self.body[2]
            return nchw(PF.ResBlockFn.apply(nhwc(x), c1.weight, c1.bias, c2.weight, c2.bias, c1.packed, c2.packed,
                                            float(self.res_scale)))
        h = nhwc(x)
        if self._bn:
            c1, b1, act, c2, b2 = self.body
            r = _conv_bn_act(c1, b1, h, act)
            r = _conv_bn_act(c2, b2, r, None)
        else:
            c1, act, c2 = self.body
            r = _conv_act(c1, h, act)
            r = _conv_act(c2, r, None)
        return nchw(PF.ScaleAddFn.apply(r, h, float(self.res_scale)))

    def _forward_attention(self, x):
        """conv + ReLU in one kernel (the ReLU's mask in the second conv's input-gradient epilogue), the second conv plain, then the
        attention node in place of the scale-and-add; the un-fused variants as in forward()."""
        h = nhwc(x)
        if self._fused:
            c1, c2 = self.body[0], self.body[2]
            r = PF.conv3x3(h, c1.weight, c1.bias, c1.packed, act=ops.ACT_RELU, relu_grad_by_consumer=True)
            t = PF.conv3x3(r, c2.weight, c2.bias, c2.packed, relu_in=True)
        elif self._bn:
            c1, b1, act, c2, b2 = self.body
            t = _conv_bn_act(c2, b2, _conv_bn_act(c1, b1, h, act), None)
        else:
            c1, act, c2 = self.body
            t = _conv_act(c2, _conv_act(c1, h, act), None)
        return nchw(self.ca(h, t, self.res_scale))


SCALES = (2, 3, 4)


class Upsampler(nn.Sequential):
    """The EDSR-style sub-pixel upsampler (reference model/basic.py:54-60 is the x4 one).
      x4: conv C->4C, PixelShuffle(2), conv C->4C, PixelShuffle(2), conv C->3 - both PixelShuffles fused into the conv
          epilogue (forward) and the dgrad/wgrad loaders (backward);
      x2: conv C->4C, PixelShuffle(2), conv C->3 - the same fused r = 2 store and loaders;
      x3: conv C->9C, PixelShuffle(3), conv C->3 - a plain conv, the standalone r = 3 kernel on its NHWC output, then the C->3
          conv (docs/modes.md section 4e).
    The convs are constructed (and draw their initialisation) in module order."""

    def __init__(self, n_feats, scale=4):
        if scale not in SCALES:
            raise ValueError(f"Upsampler: scale {scale}; supported scales are {SCALES}")
        if scale == 4:
            super().__init__(Conv(n_feats, 4 * n_feats, 3), PixelShuffle(2), Conv(n_feats, 4 * n_feats, 3), PixelShuffle(2),
                             Conv(n_feats, 3, 3))
            self[0].packed = PF.PackedConvWeights(ps=True)
            self[2].packed = PF.PackedConvWeights(ps=True)
        else:
            super().__init__(Conv(n_feats, scale * scale * n_feats, 3), PixelShuffle(scale), Conv(n_feats, 3, 3))
            if scale == 2:
                self[0].packed = PF.PackedConvWeights(ps=True)
        self.scale = scale

    def forward(self, x):
        if self.scale != 4:
            return self._forward_x2_x3(x)
        h = nhwc(x)
        h = PF.conv3x3(h, self[0].weight, self[0].bias, self[0].packed)   # -> [N, 2H, 2W, C]
        h = PF.upsample_tail(h, self[2], self[4])                         # -> [N, 4H, 4W, C] -> [N, 4H, 4W, 3]; one node (fp32)
        return nchw(h)

    def _forward_x2_x3(self, x):
        if self.scale == 2:
            return nchw(PF.upsample_tail(nhwc(x), self[0], self[2]))        # -> [N, 2H, 2W, C] (fused) -> [N, 2H, 2W, 3]; one node (fp32)
        h = PF.conv3x3(nhwc(x), self[0].weight, self[0].bias, self[0].packed)  # -> [N, H, W, 9C]
        h = _PixelShuffleRFn.apply(h, 3)                                    # -> [N, 3H, 3W, C]
        h = PF.conv3x3(h, self[2].weight, self[2].bias, self[2].packed)     # -> [N, 3H, 3W, 3]
        return nchw(h)
