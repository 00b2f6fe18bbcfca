"""Generator (EDSR-style trunk + sub-pixel upsampler: x4 as in the reference, x2 / x3 as an extension) and Discriminator (strided VGG-style stack + 2 Linear layers)
on the HIP kernels, API- and checkpoint-compatible with reference model/pesr.py: same `opt` keys, same attribute names
(`sub_mean, embed, body, upsample, add_mean` / `features, classifier`), hence the same state_dict keys and shapes, and the
same order of parameter-initialisation RNG draws.
"""
import torch
import torch.nn as nn

from .. import functional as PF
from .. import ops
from .basic import SCALES, BasicBlock, Conv, MeanShift, ResBlock, Upsampler, WindowAttention, nchw, nhwc, spectral_norm

_DIV2K_MEAN = (0.4488, 0.4371, 0.4040)      # reference model/pesr.py:13
_UNIT_STD = (1.0, 1.0, 1.0)


def discriminator_plan(first_width=64, stages=7):
    """(cin, cout, stride) of the BasicBlocks after the 3->64 stem: stride 2 on even stages, width doubling on odd ones
    (reference model/pesr.py:56-65) -> 64s2, 128, 128s2, 256, 256s2, 512, 512s2."""
    plan, width = [], first_width
    for stage in range(stages):
        if stage % 2:
            plan.append((width, 2 * width, 1))
            width *= 2
        else:
            plan.append((width, width, 2))
    return plan


def scale_of_state_dict(sd):
    """-> 2, 3 or 4: the upscaling factor of a Generator state_dict, read from its upsampler (Upsampler's table of keys and
    shapes); ValueError for anything else."""
    prefix = "module." if "module.upsample.0.weight" in sd else ""
    w0 = sd.get(prefix + "upsample.0.weight")
    if w0 is None or w0.dim() != 4:
        raise ValueError("not a Generator state_dict: no upsample.0.weight")
    if prefix + "upsample.4.weight" in sd:
        return 4
    ratio, rem = divmod(w0.shape[0], w0.shape[1])
    if rem == 0 and ratio in (4, 9) and prefix + "upsample.2.weight" in sd and sd[prefix + "upsample.2.weight"].shape[0] == 3:
        return 2 if ratio == 4 else 3
    raise ValueError(f"upsampler of unknown scale: upsample.0.weight {tuple(w0.shape)}")


def attention_of_state_dict(sd):
    """-> the reduction of a Generator state_dict's channel attention (docs/modes.md section 4u), 0 for one without: read from the
    first block's `body.0.ca.squeeze.weight` [C / reduction, C, 1, 1]; ValueError where that tensor is no such weight."""
    prefix = "module." if any(k.startswith("module.") for k in sd) else ""
    w = sd.get(prefix + "body.0.ca.squeeze.weight")
    if w is None:
        return 0
    if w.dim() != 4 or w.shape[0] < 1 or w.shape[1] % w.shape[0]:
        raise ValueError(f"channel attention of unknown shape: body.0.ca.squeeze.weight {tuple(w.shape)}")
    return w.shape[1] // w.shape[0]


def wattn_positions(every, depth):
    """The body blocks that a window-attention block follows with --wattn_every E: E - 1, 2 E - 1, ... below depth."""
    return tuple(range(every - 1, depth, every)) if every > 0 else ()


def wattn_of_state_dict(sd):
    """-> (positions, dim) of a Generator state_dict's window-attention blocks (docs/modes.md section 4w): the indices of the body
    blocks they follow, ascending, and their attention width; ((), 0) for one without.  Read from the `wattn.<i>.qkv.weight` [3 dim,
    C, 3, 3] and `wattn.<i>.proj.weight` [C, dim, 3, 3]; ValueError where these are no such weights."""
    prefix = "module." if any(k.startswith("module.") for k in sd) else ""
    head = prefix + "wattn."
    positions = sorted({k[len(head):].split(".")[0] for k in sd if k.startswith(head)}, key=lambda i: (len(i), i))
    if not positions:
        return (), 0
    dims = set()
    for i in positions:
        qkv, proj = sd.get(f"{head}{i}.qkv.weight"), sd.get(f"{head}{i}.proj.weight")
        if not i.isdigit() or qkv is None or proj is None or qkv.dim() != 4 or proj.dim() != 4 or qkv.shape[0] % 3 \
                or tuple(qkv.shape[2:]) != (3, 3) or tuple(proj.shape) != (qkv.shape[1], qkv.shape[0] // 3, 3, 3):
            raise ValueError(f"window attention of unknown shape: wattn.{i}.qkv.weight "
                             f"{None if qkv is None else tuple(qkv.shape)}, wattn.{i}.proj.weight "
                             f"{None if proj is None else tuple(proj.shape)}")
        dims.add(qkv.shape[0] // 3)
    if len(dims) != 1:
        raise ValueError(f"window attention of unknown shape: blocks of different widths {sorted(dims)}")
    return tuple(int(i) for i in positions), dims.pop()


def wattn_norm_of_state_dict(sd):
    """-> 'ln' where the window-attention blocks of a Generator state_dict carry a LayerNorm in front of qkv (docs/modes.md section 4x:
    `wattn.<i>.norm.weight` and `.bias`, both [C]), 'none' where they do not (and where there are no blocks).  ValueError where some
    blocks have one and others not, or where its tensors are not [C], C the blocks' input width."""
    prefix = "module." if any(k.startswith("module.") for k in sd) else ""
    head = prefix + "wattn."
    positions = sorted({k[len(head):].split(".")[0] for k in sd if k.startswith(head)}, key=lambda i: (len(i), i))
    with_norm = [i for i in positions if any(k.startswith(f"{head}{i}.norm.") for k in sd)]
    if not with_norm:
        return 'none'
    if len(with_norm) != len(positions):
        raise ValueError(f"window attention of unknown shape: the blocks {with_norm} have a norm, "
                         f"{[i for i in positions if i not in with_norm]} have none")
    for i in positions:
        qkv, w, b = sd.get(f"{head}{i}.qkv.weight"), sd.get(f"{head}{i}.norm.weight"), sd.get(f"{head}{i}.norm.bias")
        want = None if qkv is None or qkv.dim() != 4 else (qkv.shape[1],)
        if w is None or b is None or want is None or tuple(w.shape) != want or tuple(b.shape) != want:
            raise ValueError(f"window attention of unknown shape: wattn.{i}.norm.weight {None if w is None else tuple(w.shape)}, "
                             f"wattn.{i}.norm.bias {None if b is None else tuple(b.shape)}; expected {want} for both")
    return 'ln'


class Generator(nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.opt = dict(opt)               # (what a second Generator of this shape is built from: FlatAdam.ema_module)
        width, depth, res_scale = opt['num_channels'], opt['depth'], opt['res_scale']
        scale = opt.get('scale', 4)        # an extension: the reference's Generator is x4 only (docs/modes.md section 4e)
        if scale not in SCALES:
            raise ValueError(f"Generator: scale {scale}; supported scales are {SCALES}")
        # an extension: channel attention in the residual blocks (docs/modes.md section 4u); absent or None = the reference's blocks
        attention, reduction = opt.get('attention'), opt.get('ca_reduction', 16)
        block_kw = {} if attention is None else {"attention": attention, "reduction": reduction}
        # The reference builds the trunk before everything else (RNG order) but registers it third (state_dict order).
        trunk = [ResBlock(width, 3, act=nn.ReLU(True), res_scale=res_scale, **block_kw) for _ in range(depth)]
        trunk.append(Conv(width, width, 3))
        self.sub_mean = MeanShift(255, _DIV2K_MEAN, _UNIT_STD)
        self.embed = Conv(3, width, 3)
        self.body = nn.Sequential(*trunk)
        self.upsample = Upsampler(width, scale)
        self.add_mean = MeanShift(255, _DIV2K_MEAN, _UNIT_STD, 1)
        # an extension: a window self-attention block after every wattn_every-th residual block (docs/modes.md section 4w), keyed by the
        # index of that block, shifted by half a window at every second one.  Constructed and registered after everything else: every
        # other parameter keeps its initial value and its key.  Absent or 0 = nothing is built.
        every, dim = opt.get('wattn_every', 0) or 0, opt.get('wattn_dim') or width // 2
        if every < 0 or every > depth:
            raise ValueError(f"Generator: wattn_every = {every}; expected 0 (off) .. depth = {depth}")
        # an extension of that extension: a LayerNorm over each pixel's channels in front of every block's qkv (docs/modes.md section
        # 4x); absent, None or 'none' = the blocks as they were.  It draws nothing from the RNG.
        norm = opt.get('wattn_norm')
        if norm not in (None, 'none', 'ln'):
            raise ValueError(f"Generator: wattn_norm = {norm!r}; expected None, 'none' or 'ln'")
        if norm == 'ln' and not every:
            raise ValueError("Generator: wattn_norm = 'ln' without wattn_every: there is no window-attention block to normalise")
        if every:
            self.wattn = nn.ModuleDict({str(i): WindowAttention(width, dim, shift=4 * (j % 2), norm="ln" if norm == 'ln' else None)
                                        for j, i in enumerate(wattn_positions(every, depth))})

    def forward(self, x):
        feat = self.embed(self.sub_mean(x))
        h = feat
        wattn = getattr(self, "wattn", None)
        for i, block in enumerate(self.body[:-1]):
            h = block(h)
            if wattn is not None and str(i) in wattn:
                h = wattn[str(i)](h)
        last = self.body[-1]
        # trunk tail conv and the global skip (`res += x`, reference model/pesr.py:32-33) in one kernel
        h = nchw(PF.ConvAddFn.apply(nhwc(h), nhwc(feat), last.weight, last.bias, last.packed))
        return self.add_mean(self.upsample(h))


class Discriminator(nn.Module):
    def __init__(self, opt):
        super().__init__()
        lrelu = nn.LeakyReLU(negative_slope=0.2, inplace=True)
        use_sn = opt['spectral_norm']
        blocks = [BasicBlock(3, 64, 3, bn=True, act=lrelu, sn=use_sn)]
        for cin, cout, stride in discriminator_plan():
            blocks.append(BasicBlock(cin, cout, 3, stride=stride, bn=True, act=lrelu, sn=use_sn))
        self.features = nn.Sequential(*blocks)
        # the last block emits NCHW-contiguous so that .view(B, -1) has the reference's column order (c, y, x)
        self.features[-1].flatten_output = True
        side = (opt['patch_size'] * opt.get('scale', 4)) // 16   # four stride-2 stages on the HR patch (scale x the LR patch)
        self.classifier = nn.Sequential(nn.Linear(512 * side * side, 1024), lrelu, nn.Linear(1024, 1))

    def forward_features(self, x):
        """The eight conv + BatchNorm + LeakyReLU blocks: [B, 3, H, W] -> [B, 512 * side * side] in the reference's NCHW column order
        (reference model/pesr.py:78-79).  One call = one set of BatchNorm batch statistics, as in the reference."""
        # the blocks are chained here (not through nn.Sequential.forward) so that each block knows its producer: the tensors in between
        # are seen by nobody else, which lets a block's input-gradient kernel do the BatchNorm reductions of the block in front of it
        flat, link = x, None
        for blk in self.features:
            flat, link = blk.forward_linked(flat, link) if isinstance(blk, BasicBlock) else (blk(flat), None)
        return flat.view(flat.size(0), -1)

    def classify(self, flat, grad_rows=None):
        """Linear -> LeakyReLU -> Linear (reference model/pesr.py:69-75,80) on the flattened features.  The classifier has no BatchNorm,
        so its rows are independent: the train step hands it the features of TWO calls at once ([hr; sr]) and the 302 MB weight matrix
        of classifier.0 is streamed once instead of twice, forward and backward (pesr_amd.step.Trainer.gan_step).  grad_rows: only the
        first grad_rows rows need an input gradient (functional.LinearFn)."""
        fc1, act, fc2 = self.classifier
        hidden = PF.LinearFn.apply(flat, fc1.weight, fc1.bias, ops.ACT_LRELU, act.negative_slope, grad_rows)
        return PF.LinearFn.apply(hidden, fc2.weight, fc2.bias, ops.ACT_NONE, 0.0)

    PAIR_ROWS = 16   # rows per call inside a paired classifier pass: the Linear kernels add rows in chains of sixteen (linear.hip)

    def classify_pair(self, fa, fb, grad_first_only=False):
        """classify() of two calls' features in ONE pass over the weights: -> (logits of fa, logits of fb).  Each call takes a block of
        sixteen rows (shorter batches are padded with zero rows, which add exact zeros), and the kernels sum every block as a chain of its
        own before adding the blocks - so forward values, input gradients, weight and bias gradients are bit for bit those of two
        separate calls.  Batches above sixteen: call classify() twice.  grad_first_only: fb came from a no_grad pass."""
        B, R = fa.shape[0], self.PAIR_ROWS
        assert fb.shape == fa.shape and B <= R
        if B < R:
            pad = fa.new_zeros((R - B, fa.shape[1]))
            x = torch.cat([fa, pad, fb, pad])
        else:
            x = torch.cat([fa, fb])
        preds = self.classify(x, grad_rows=R if grad_first_only else None)
        return PF.SplitRowsFn.apply(preds, B, R)

    def forward(self, x):
        return self.classify(self.forward_features(x))


class UNetDiscriminator(nn.Module):
    """A U-Net discriminator with spectral norm that emits one logit per pixel (an extension, docs/modes.md section 4v): Real-ESRGAN's
    `UNetDiscriminatorSN` (Wang et al., ICCVW 2021, after Schoenfeld et al., CVPR 2020) with ONE deviation - its three 4 x 4 stride-2
    convs are 3 x 3 stride-2 here (the MFMA stride-2 kernels are 3 x 3 and Conv refuses even sizes), so its published weights do not load.
    [B, 3, H, W] with H, W multiples of 8 -> [B, 1, H, W]; independent of opt['patch_size'].  w = opt.get('d_width', 64):
        conv0 3 -> w (bias)                       lrelu -> x0          conv4 8w -> 4w on up2(x3)   lrelu, + x2 -> x4
        conv1 w -> 2w, conv2 -> 4w, conv3 -> 8w,                       conv5 4w -> 2w on up2(x4)   lrelu, + x1 -> x5
              stride 2                            lrelu -> x1, x2, x3  conv6 2w -> w  on up2(x5)   lrelu, + x0 -> x6
        conv7, conv8 w -> w   lrelu                                    conv9 w -> 1 (bias)         the logits
    LeakyReLU(0.2), no BatchNorm; conv1 .. conv8 have no bias and, with opt['spectral_norm'], spectral norm (torch's state_dict schema).
    up2 = bilinear x2; it is linear, so the additions `+ x2`, `+ x1` run inside the upsample kernel that follows them.  The convs are
    constructed (and draw their nn.Conv2d default initialisation, then u and v) in the order conv0 .. conv9."""

    def __init__(self, opt):
        super().__init__()
        w = opt.get('d_width', 64)
        if w < 4 or w % 4:
            raise ValueError(f"UNetDiscriminator: d_width = {w}; a positive multiple of 4 (train.py asks for a multiple of 16)")
        sn = (lambda c: spectral_norm(c)) if opt['spectral_norm'] else (lambda c: c)
        self.slope = 0.2
        self.conv0 = Conv(3, w, 3)
        self.conv1 = sn(Conv(w, 2 * w, 3, stride=2, bias=False))
        self.conv2 = sn(Conv(2 * w, 4 * w, 3, stride=2, bias=False))
        self.conv3 = sn(Conv(4 * w, 8 * w, 3, stride=2, bias=False))
        self.conv4 = sn(Conv(8 * w, 4 * w, 3, bias=False))
        self.conv5 = sn(Conv(4 * w, 2 * w, 3, bias=False))
        self.conv6 = sn(Conv(2 * w, w, 3, bias=False))
        self.conv7 = sn(Conv(w, w, 3, bias=False))
        self.conv8 = sn(Conv(w, w, 3, bias=False))
        self.conv9 = Conv(w, 1, 3)
        self.width = w

    def _act(self, conv, h):
        return PF.ConvLReluFn.apply(h, conv.effective_weight(), conv.bias, conv.packed, conv.stride, self.slope)

    def forward(self, x):
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] < 8 or x.shape[3] < 8 or x.shape[2] % 8 or x.shape[3] % 8:
            raise ValueError(f"UNetDiscriminator: input {tuple(x.shape)}; expected [B, 3, H, W] with H and W multiples of 8 (three "
                             f"stride-2 stages and their x2 upsamplings)")
        x0 = self._act(self.conv0, nhwc(x))
        x1 = self._act(self.conv1, x0)
        x2 = self._act(self.conv2, x1)
        x3 = self._act(self.conv3, x2)
        t4 = self._act(self.conv4, PF.BilinearUp2Fn.apply(x3))
        t5 = self._act(self.conv5, PF.BilinearUp2Fn.apply(t4, x2))        # up2(x4), x4 = t4 + x2
        t6 = self._act(self.conv6, PF.BilinearUp2Fn.apply(t5, x1))        # up2(x5), x5 = t5 + x1
        x6 = PF.ScaleAddFn.apply(t6, x0, 1.0)
        h = self._act(self.conv8, self._act(self.conv7, x6))
        c9 = self.conv9
        return nchw(PF.conv3x3(h, c9.weight, c9.bias, c9.packed))

    def forward_features(self, *a, **k):
        raise TypeError("UNetDiscriminator has no feature / classifier split: call it as a whole (the paired-classifier path of "
                        "Trainer.gan_step applies to Discriminator only)")

    classify = classify_pair = forward_features


D_ARCHS = ("vgg", "unet")


def build_discriminator(opt, d_arch="vgg"):
    """train.py --d_arch: "vgg" - the reference's Discriminator(opt), constructed exactly as without the argument; "unet" - the
    UNetDiscriminator(opt) (opt['d_width'], docs/modes.md section 4v)."""
    if d_arch not in D_ARCHS:
        raise ValueError(f"build_discriminator: d_arch = {d_arch!r}; one of {D_ARCHS}")
    return UNetDiscriminator(opt) if d_arch == "unet" else Discriminator(opt)


def _forward_second_order(self, x):
    """D(x) through twice-differentiable, un-fused functions (pesr_amd.functional *2Fn): the extra forward of the gradient
    penalty (reference train.py:216-226), whose result goes into torch.autograd.grad(..., create_graph=True).  Same values as
    forward() up to fp32 rounding; BatchNorm runs in training mode and updates its running statistics like any other call."""
    h = nhwc(x)
    for blk in self.features:
        conv, bn, act = blk[0], blk[1], blk[2]
        z = PF.Conv2Fn.apply(h, conv.effective_weight(), conv.packed, conv.stride)
        u = PF.Bn2Fn.apply(z, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.eps, bn.momentum)
        h = PF.LRelu2Fn.apply(u, float(act.negative_slope))
    flat = nchw(h).contiguous().view(h.size(0), -1)          # NCHW flatten (reference model/pesr.py:79)
    fc1, act, fc2 = self.classifier
    hidden = PF.LRelu2Fn.apply(PF.Linear2Fn.apply(flat, fc1.weight, fc1.bias), float(act.negative_slope))
    return PF.Linear2Fn.apply(hidden, fc2.weight, fc2.bias)


Discriminator.forward_second_order = _forward_second_order
