"""Autograd glue over the HIP ops: one torch.autograd.Function per fused block of the reference graph.

Tensors crossing these functions are NHWC-contiguous fp32 GPU tensors ([N, H, W, C]); the nn.Modules in
pesr_amd/model convert from/to the logical NCHW view at the network boundary only.  Nothing here does
arithmetic in torch except scalar-sized glue (gradient fan-in adds are autograd's own).
"""
from __future__ import annotations

import os
import threading
import weakref

import torch
from torch.autograd import Function

from . import ops

# Our fused Adam writes parameters through raw pointers and cannot bump Tensor._version, so every parameter it owns
# carries an explicit epoch (bumped by FlatAdam.step for ITS parameters only - the static VGG weights and the other
# network's weights keep their packed copies).  Part of every packed-weight cache key.  The epoch is an attribute of the
# parameter object itself: it lives and dies with the parameter (a registry keyed by id() would outlive it and hand a
# recycled id a dead optimizer's state).
_EPOCH_ATTR = "_pesr_epoch"
_GRAD_VIEW_ATTR = "_pesr_grad_view"


def weight_epoch(p) -> int:
    return getattr(p, _EPOCH_ATTR, 0)


def bump_weight_epoch(params) -> None:
    for p in params:
        setattr(p, _EPOCH_ATTR, getattr(p, _EPOCH_ATTR, 0) + 1)


# Flat-gradient fast path.  pesr_amd.optim.FlatParams registers, per parameter, a factory of fresh views into its flat
# gradient buffer.  When a backward produces a parameter's FIRST gradient of the step (param.grad is None) the kernel
# writes straight into such a view and returns it; autograd then adopts it as .grad without a copy or an add kernel
# (AccumulateGrad steals a uniquely-referenced, contiguous gradient).  The slice is handed out ONCE per step: a
# parameter used twice in one graph (the Discriminator sees hr and sr in the same backward) gets a temporary for its
# second contribution, which autograd's input buffer adds to the first.  Stored as [factory, claimed] on the parameter
# object (same lifetime argument as the epoch); the factory holds only a weak reference to its FlatParams.
def register_grad_view(param: torch.Tensor, factory) -> None:
    setattr(param, _GRAD_VIEW_ATTR, [factory, False])


def unregister_grad_view(param: torch.Tensor) -> None:
    if hasattr(param, _GRAD_VIEW_ATTR):
        delattr(param, _GRAD_VIEW_ATTR)


def release_grad_views(params) -> None:
    """New step (zero_grad): every registered slice may be claimed again."""
    for p in params:
        e = getattr(p, _GRAD_VIEW_ATTR, None)
        if e is not None:
            e[1] = False


def grad_out_again(param):
    """The parameter's flat-gradient slice AFTER it has been claimed in this step (by grad_out), for a kernel that can
    accumulate into it - the second use of a layer inside one backward pass; else None."""
    if param is None or not param.is_leaf:
        return None
    e = getattr(param, _GRAD_VIEW_ATTR, None)
    if e is None or not e[1]:
        return None
    return e[0]()


def grad_view_claimed(param) -> bool:
    e = getattr(param, _GRAD_VIEW_ATTR, None)
    return bool(e is not None and e[1])


def grad_out(param):
    """A fresh view of the parameter's flat-gradient slice if its first gradient may be written there, else None."""
    if param is None or not param.is_leaf or param.grad is not None:      # (replicas of nn.DataParallel are non-leaf)
        return None
    e = getattr(param, _GRAD_VIEW_ATTR, None)
    if e is None or e[1]:
        return None
    view = e[0]()
    if view is None:          # the owning FlatParams is gone
        return None
    e[1] = True
    return view


_ALL_PACKS = []   # weak registry of every PackedConvWeights (for the batched repack after an optimizer step)


class _PackSlot:
    """The packed layouts of one weight tensor ON ONE DEVICE: packs[mode] = [packed, key of the tensor it was built from], under the
    batched re-pack's mode numbers (csrc/pack.hip) - family.mode of ops._FAMILIES for the forward packing, + 1 for the dgrad one."""
    __slots__ = ("packs", "wref", "bref")

    def __init__(self):
        self.packs = {}
        self.wref = None            # weakref to the weight tensor this slot was last built from
        self.bref = None            # ... and to the bias tensor of its PixelShuffle-permuted copy (packs[_BIAS])


_BIAS = 6       # the slot of the PixelShuffle-permuted bias: no mode of the batched kernel, a number in this bookkeeping only


class PackedConvWeights:
    """Per-module cache of the kernel-side weight layouts (forward / dgrad packing of each kernel family used, PS-permuted bias).

    One slot per device: nn.DataParallel's replicas are shallow copies that SHARE this object while their weights live
    on different GPUs and their forwards run on concurrent threads (SURVEY 8b "Threading") - every replica works on its
    own device's slot, and the lock makes the check-then-pack step atomic."""

    def __init__(self, ps: bool = False):
        self.ps = ps
        self._slots = {}            # device index -> _PackSlot
        self._lock = threading.Lock()
        _ALL_PACKS.append(weakref.ref(self))

    def __deepcopy__(self, memo):   # copy.deepcopy(module): a fresh, empty cache (locks cannot be copied)
        return PackedConvWeights(self.ps)

    def __getstate__(self):         # pickling a module (torch.save(model)): drop the device buffers and the lock
        return {"ps": self.ps}

    def __setstate__(self, st):
        self.__init__(st["ps"])

    @staticmethod
    def _key(t: torch.Tensor):
        return (t.data_ptr(), t._version, weight_epoch(t))

    def _slot(self, t) -> _PackSlot:
        idx = t.device.index if t.is_cuda else -1
        sl = self._slots.get(idx)
        if sl is None:
            sl = self._slots[idx] = _PackSlot()
        return sl

    def _get(self, w, family, dgrad: int):
        assert tuple(w.shape[2:]) == (3, 3), f"PackedConvWeights: 3x3 kernels only, got a weight of shape {tuple(w.shape)}"
        mode = family.mode + dgrad
        with self._lock:
            sl = self._slot(w)
            if sl.wref is None or sl.wref() is not w:
                sl.wref = weakref.ref(w)
            k = self._key(w)
            e = sl.packs.get(mode)
            if e is None or e[1] != k:
                e = sl.packs[mode] = [ops._pack(family, w.detach(), dgrad, self.ps), k]
            return e[0]

    def for_fwd(self, w: torch.Tensor, x_shape, stride: int = 1):
        """Packed weights for y = conv(x, w) with x of NHWC shape x_shape: of the first kernel family in ops._FAMILIES that applies and
        fills the chip."""
        return self._get(w, ops.conv3x3_family_fwd(*x_shape, w.shape[0], stride, self.ps), 0)

    def for_dgrad(self, w: torch.Tensor, x_shape, stride: int = 1):
        """Packed weights for dx of that conv."""
        return self._get(w, ops.conv3x3_family_dgrad(*x_shape, w.shape[0], stride, self.ps), 1)

    def bias(self, b):
        if b is None or not self.ps:
            return None if b is None else b.detach()
        with self._lock:
            sl = self._slot(b)
            k = self._key(b)
            e = sl.packs.get(_BIAS)
            if e is None or e[1] != k:
                e = sl.packs[_BIAS] = [ops.pack_bias_ps(b.detach()), k]
            if sl.bref is None or sl.bref() is not b:
                sl.bref = weakref.ref(b)
            return e[0]


# Optional side stream for the weight-gradient kernels (off by default): in a backward chain the dgrad kernels
# depend on each other but the wgrad kernels only consume their outputs, so with two streams the workgroups of a wgrad can
# fill the CUs that the previous dgrad frees during its tail.  It paid with the direct kernels; with the Winograd kernels
# the fork / join costs more than the tails it fills.
_SIDE = {}
# PESR_SIDE_STREAM: "0" everything on one stream, "1" every conv block's wgrad on the side stream, "g" only the blocks
# without BatchNorm (the Generator's), "d" only the conv+BN blocks (the Discriminator's)
SIDE_MODE = os.environ.get("PESR_SIDE_STREAM", "0")
USE_SIDE_STREAM = SIDE_MODE != "0"
_SIDE_OFF = SIDE_MODE == "0"     # (in-place second-use accumulation assumes every weight gradient is written on ONE stream)


def side_stream(device) -> "torch.cuda.Stream":
    s = _SIDE.get(device.index)
    if s is None:
        s = _SIDE[device.index] = torch.cuda.Stream(device=device)
    return s


def join_side_stream(device=None) -> None:
    """Make the current stream wait for everything queued on the side stream (optimizer step, gradient all-reduce)."""
    for idx, s in _SIDE.items():
        if device is None or device.index == idx:
            torch.cuda.current_stream(s.device).wait_stream(s)


_JOIN_QUEUED = [False]


def _join_after_backward():
    _JOIN_QUEUED[0] = False
    join_side_stream()


class _OnSide:
    """with _OnSide(dev, tensors...): the side stream first waits for the work queued so far on the current stream;
    the listed tensors (inputs read on the side stream) are protected from the caching allocator's early reuse.

    Stream safety of the RESULTS: a gradient written into a flat-gradient view (`fast`) is consumed only by code that
    joins the side stream first (FlatAdam.step, the all-reduce buckets, and a callback queued at the end of every
    backward pass).  Anything else - a temporary that autograd itself will add to another contribution on the main
    stream - makes the main stream wait for the side stream on exit (`fast=False`)."""

    def __init__(self, device, *tensors, fast=False, where="g"):
        self.enabled = where is not None and (SIDE_MODE == "1" or SIDE_MODE == where)      # where=None: a node without a side stream
        self.fast, self.device = fast, device
        if self.enabled:
            if not _JOIN_QUEUED[0]:
                try:
                    torch.autograd.Variable._execution_engine.queue_callback(_join_after_backward)
                    _JOIN_QUEUED[0] = True
                except RuntimeError:      # not inside a backward pass (direct call of a backward in a test)
                    self.fast = False
            self.side = side_stream(device)
            self.side.wait_stream(torch.cuda.current_stream(device))
            for t in tensors:
                if t is not None:
                    t.record_stream(self.side)
            self.ctx = torch.cuda.stream(self.side)

    def __enter__(self):
        if self.enabled:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.enabled:
            self.ctx.__exit__(*a)
            if not self.fast:
                torch.cuda.current_stream(self.device).wait_stream(self.side)


_REPACK_TABLES = {}        # key -> device descriptor table, least recently used first (a dict keeps insertion order)
_REPACK_TABLES_MAX = 8
# Set (to a list) by Trainer._capture while a step is being captured into a hipGraph: every repack_all launch under capture
# appends (jobs, table).  The graph holds the table's and the packed buffers' RAW pointers, so the capture state keeps these
# objects alive (an evicted table, or a packed buffer an eager rebuild replaced, would otherwise go back to the caching
# allocator and the next replay would read / write reused memory), and Trainer._replay uses the job list to re-stamp exactly
# the packings the replayed launch refreshed.
_REPACK_RECORD = None

def stamp_repacked(jobs) -> None:
    """Mark the packings of `jobs` (as recorded by repack_all) as built from their weights' CURRENT contents.  A packing whose
    buffer is no longer the recorded one (an eager rebuild replaced it) is left alone: its key then misses and it is rebuilt
    on next use."""
    for sl, wref, mode, ptr in jobs:
        w = wref()          # (mode _BIAS: the bias tensor)
        e = sl.packs.get(mode)
        if w is not None and e is not None and e[0].data_ptr() == ptr:
            e[1] = PackedConvWeights._key(w)


def repack_all(params) -> None:
    """Refresh, in ONE kernel launch, every packed layout that already exists for the given parameters (called by
    FlatAdam.step right after its Adam kernel, instead of ~2 small pack launches per conv on the next forward/backward)."""
    import numpy as np
    ids = {id(p) for p in params}
    jobs, bias_rec = [], []
    for ref in list(_ALL_PACKS):
        c = ref()
        if c is None:
            _ALL_PACKS.remove(ref)
            continue
        for sl in list(c._slots.values()):
            w = sl.wref() if sl.wref is not None else None
            b = sl.bref() if sl.bref is not None else None
            for mode, (packed, _) in sorted(sl.packs.items()):
                if mode == _BIAS:
                    # PixelShuffle-permuted biases of these parameters: refreshed in place too (two tiny launches for the Generator).
                    # Left to the lazy per-forward check they were re-packed on every forward - and a captured step whose capture
                    # happened to find the key current (a forward between the last optimizer step and the capture) would never
                    # refresh them at all.
                    if b is not None and id(b) in ids and b.is_cuda:
                        ops.pack_bias_ps(b.detach(), out=packed)
                        bias_rec.append((sl, sl.bref, _BIAS, packed.data_ptr()))
                elif w is not None and id(w) in ids and w.is_cuda:
                    O, I = w.shape[0], w.shape[1]
                    f = ops._conv_family(packed)
                    jobs.append((sl, w, mode, (w.data_ptr(), packed.data_ptr(), O, I, mode, int(c.ps), *f.dims(O, I, mode - f.mode))))
    if bias_rec:
        if _REPACK_RECORD is not None:
            _REPACK_RECORD.append((bias_rec, None, [sl.packs[_BIAS][0] for sl, _, _, _ in bias_rec]))
        stamp_repacked(bias_rec)
    if not jobs:
        return
    dev = jobs[0][1].device
    key = (tuple(sorted(ids)), tuple(j[3] for j in jobs))
    # One descriptor table per (parameter set, pack layout), kept on the device: the H2D copy that builds it SYNCHRONISES the
    # host with the stream, so it must happen once per optimizer - not once per step (with one shared slot, the G and D
    # optimizers of the GAN step evicted each other's table every step and the host could never run ahead of the GPU).
    table = _REPACK_TABLES.pop(key, None)
    if table is None:
        while len(_REPACK_TABLES) >= _REPACK_TABLES_MAX:           # least recently used goes first
            _REPACK_TABLES.pop(next(iter(_REPACK_TABLES)))
        table = torch.from_numpy(np.array([j[3] for j in jobs], dtype=np.int64)).to(dev)
    _REPACK_TABLES[key] = table                                    # (re-)inserted as the most recently used
    from . import _lib
    _lib.check(_lib.lib().pesr_pack_conv3x3_batched(table.data_ptr(), len(jobs), torch.cuda.current_stream(dev).cuda_stream),
               "pesr_pack_conv3x3_batched")
    rec = [(sl, weakref.ref(w), mode, d[1]) for sl, w, mode, d in jobs]
    if _REPACK_RECORD is not None:
        # under capture nothing ran: the record (it also pins the table and the packed buffers) is used at replay time
        _REPACK_RECORD.append((rec, table, [sl.packs[mode][0] for sl, _, mode, _ in jobs]))
    stamp_repacked(rec)


def _c(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------------------------
# The routing of every 3x3 conv node: which kernel runs its forward, its input gradient and its weight gradient.  The nodes
# below keep the bookkeeping that is their own (saved tensors, masks, needs_input_grad) and call these three.
# ------------------------------------------------------------------------------------------------
def _conv_fwd(x, weight, bias, cache, stride=1, **epilogue):
    """y = epilogue(conv(x, weight) + bias); epilogue: act, slope, alpha, skip, mask of ops.conv3x3_fwd.  The pack is lazy (it is the
    launch right before the kernel that reads it, and none when an RGB kernel runs on the OIHW weights)."""
    return ops.conv3x3_fwd(x, lambda: cache.for_fwd(weight, x.shape, stride), cache.bias(bias), weight.shape[0], stride,
                           ps_out=cache.ps, w_oihw=weight.detach(), **epilogue)


def _conv_wgrad(x, gy, weight, bias_ref, stride, ps, want_w, want_b, *, alpha=1.0, where=None, again=None):
    """(dw, db) of y = conv(x, weight) + bias: the RGB kernel where one side has three channels, else ops.conv3x3_wgrad; a parameter's
    first gradient of the step is written into its flat-gradient view (grad_out; plain tensors have none).  where: the SIDE_MODE under
    which this node's weight gradient runs on the side stream (None: never).  again: the (weight, bias) views _second_use returned -
    the gradient is added to them on the current stream and autograd gets (None, None)."""
    if not want_w:
        return None, None
    if again is not None:
        (o_w, o_b), where = again, None
        want_b = o_b is not None
    else:
        o_w, o_b = grad_out(weight), grad_out(bias_ref) if want_b else None
    kw = dict(alpha=alpha, want_bias=want_b, dw_out=o_w, db_out=o_b, accumulate=again is not None)
    side = ops.wgrad_rgb_side(x.shape[3], weight.shape[0])
    with _OnSide(gy.device, x, gy, fast=o_w is not None and (o_b is not None or not want_b), where=where):
        if ops.c1_eligible(x.shape[3], weight.shape[0], stride):     # C -> 1: its own kernels (csrc/conv_c1.hip)
            if again is not None:
                raise NotImplementedError("the C -> 1 weight gradient has no accumulating form: a node that adds a second use in "
                                          "place (_second_use) cannot hold a one-channel conv")
            dw, db = ops.conv3x3_c1_wgrad(x, gy, alpha=alpha, want_bias=want_b, dw_out=o_w, db_out=o_b)
        elif side is None:
            dw, db = ops.conv3x3_wgrad(x, gy, stride, ps_in=ps, **kw)
        else:
            dw, db = ops.conv3x3_wgrad_rgb(gy, x, 0, **kw) if side == 0 else ops.conv3x3_wgrad_rgb(x, gy, 1, **kw)
    return (None, None) if again is not None else (dw, db)


def _dgrad_pack(weight, cache, x_shape, stride, plain=True):
    """The packed weights _conv_dgrad will run on, or None where one of the two HBM-bound RGB kernels runs on the OIHW weights: dx of a
    C -> 3 conv is a 3 -> C conv of dy, dx of a 3 -> C conv a C -> 3 conv of dy (plain: no fused mask / skip / scale, which they lack).
    Nodes that pack before their weight gradient (packing happens on the main stream) call this first and hand the result on."""
    cin, cout = x_shape[3], weight.shape[0]
    if plain and not cache.ps and (ops.rgb_in_eligible(cout, cin, stride) or ops.rgb_in_dgrad_eligible(cin, cout, stride) or
                                   ops.c1_eligible(cin, cout, stride)):
        return None
    return cache.for_dgrad(weight, x_shape, stride)


_PACK_NOW = object()


def _conv_dgrad(gy, weight, cache, x_shape, stride=1, *, mask=None, skip=None, alpha=1.0, prev_link=None, wpd=_PACK_NOW):
    """dx = alpha * dgrad(gy) [masked by mask > 0] [+ skip].  prev_link: x is the output of a BatchNorm + LeakyReLU block (BnLink): where
    the kernel can, it folds that block's backward reductions into its epilogue and leaves them in the link.  wpd: the answer of an
    earlier _dgrad_pack."""
    x_shape = tuple(x_shape)
    if wpd is _PACK_NOW:
        wpd = _dgrad_pack(weight, cache, x_shape, stride, mask is None and skip is None and alpha == 1.0)
    if wpd is None and weight.shape[0] == 1:
        return ops.conv3x3_c1_dgrad(gy, weight.detach(), x_shape)
    if wpd is None:
        return (ops.conv3x3_rgb_in_dgrad if x_shape[3] == 3 else ops.conv3x3_rgb_dgrad)(gy, weight.detach(), x_shape)
    if prev_link is not None and prev_link.z is not None:
        res = ops.conv3x3_dgrad_bn_sums(gy, wpd, x_shape, stride, prev_link.z, prev_link.stats, prev_link.gamma, prev_link.beta, prev_link.slope)
        if res is not None:
            dx, prev_link.part = res
            prev_link.g_ptr = dx.data_ptr()
            return dx
    return ops.conv3x3_dgrad(gy, wpd, x_shape, stride, alpha=alpha, mask=mask, skip=skip, ps_in=cache.ps)


def _second_use(params, allowed, grad_free):
    """The SECOND use of a layer inside one backward pass (the Discriminator sees hr and sr in one graph, reference train.py:205-214) may
    add its parameter gradients to the flat-gradient slices the first use wrote, so that autograd gets nothing to add: -> the claimed
    views of `params`, or None when it may not.  allowed: the conditions of the calling node; grad_free: the parameters that must not
    have a .grad yet.  See INPLACE_SECOND_USE for when the whole protocol is off."""
    if not (INPLACE_SECOND_USE and allowed):
        return None
    views = [grad_out_again(p) for p in params]        # (None for a parameter that is no leaf, has no slice or has not claimed it)
    return None if any(v is None for v in views) or any(p.grad is not None for p in grad_free) else views


# ------------------------------------------------------------------------------------------------
# generic 3x3 conv (+bias, +ReLU, fused PixelShuffle)          reference model/basic.py:4-7, 56-60
# ------------------------------------------------------------------------------------------------
class Conv3x3Fn(Function):
    """y = act(conv(x, w) + b) [pixel-shuffled].

    relu_in:  x is the output of a ReLU whose backward this function applies to its grad_input
              (mask by x > 0, fused in the dgrad epilogue).
    relu_grad_by_consumer: with act=relu, the consumer of y applies the ReLU mask (it set relu_in);
              otherwise this function masks grad_output itself.
    precision: None - forward and backward dispatch by ops.PRECISION as it is when each runs (every network's own nodes); a mode - both
              run under that mode whatever is set then (the LPIPS trunk inside a bf16 step: its backward runs later, inside
              total_G_loss.backward(), docs/modes.md section 4o).
    """

    @staticmethod
    def forward(ctx, x, weight, bias, cache: PackedConvWeights, stride, act, relu_in, relu_grad_by_consumer, precision=None):
        x = _c(x)
        with ops.use_precision(precision):
            y = _conv_fwd(x, weight, bias, cache, stride, act=act)
        ctx.precision = precision
        ctx.cache, ctx.stride, ctx.act, ctx.relu_in = cache, stride, act, relu_in
        ctx.mask_here = act == ops.ACT_RELU and not relu_grad_by_consumer
        ctx.has_bias = bias is not None
        ctx.bias_ref = bias
        ctx.save_for_backward(x, weight, y if ctx.mask_here else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, y = ctx.saved_tensors
        gy = _c(gy)
        if ctx.mask_here:
            gy = ops.relu_mask(gy, y)
        need_dx = ctx.needs_input_grad[0]
        with ops.use_precision(ctx.precision):
            wpd = _dgrad_pack(weight, ctx.cache, x.shape, ctx.stride, not ctx.relu_in) if need_dx else None
            dw, db = _conv_wgrad(x, gy, weight, ctx.bias_ref, ctx.stride, ctx.cache.ps, ctx.needs_input_grad[1],
                                 ctx.has_bias and ctx.needs_input_grad[2], where="g")
            dx = _conv_dgrad(gy, weight, ctx.cache, x.shape, ctx.stride, mask=x if ctx.relu_in else None, wpd=wpd) if need_dx else None
        return dx, dw, db, None, None, None, None, None, None


class ConvLReluFn(Function):
    """y = leaky_relu(conv(x, w) + b, slope): BasicBlock(bn=False, act=LeakyReLU) / ResBlock(act=LeakyReLU) - constructor
    branches of reference model/basic.py the reference's own scripts never take."""

    @staticmethod
    def forward(ctx, x, weight, bias, cache, stride, slope):
        x = _c(x)
        y = _conv_fwd(x, weight, bias, cache, stride, act=ops.ACT_LRELU, slope=slope)
        ctx.cache, ctx.stride, ctx.slope, ctx.bias_ref = cache, stride, slope, bias
        ctx.save_for_backward(x, weight, y)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, y = ctx.saved_tensors
        gz = ops.relu_mask(_c(gy), y, slope=ctx.slope)          # sign(y) == sign(z) for a positive slope
        dw, db = _conv_wgrad(x, gz, weight, ctx.bias_ref, ctx.stride, ctx.cache.ps, ctx.needs_input_grad[1],
                             ctx.bias_ref is not None and ctx.needs_input_grad[2])
        dx = _conv_dgrad(gz, weight, ctx.cache, x.shape, ctx.stride) if ctx.needs_input_grad[0] else None
        return dx, dw, db, None, None, None


class ConvKxKFn(Function):
    """y = conv(x, w) + b for an odd kernel size other than 3 (reference model/basic.py:4-7 accepts any; its networks use 3 only):
    the generic, untuned kernels of conv_kxk.hip.  Activations are applied by the caller (ops.relu_mask)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride):
        x = _c(x)
        ctx.stride, ctx.bias_ref = stride, bias
        ctx.save_for_backward(x, weight)
        return ops.conv_kxk_fwd(x, _c(weight.detach()), None if bias is None else bias.detach(), stride)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = _c(gy)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = ops.conv_kxk_dgrad(gy, _c(weight.detach()), tuple(x.shape), ctx.stride)
        if ctx.needs_input_grad[1]:
            want_b = ctx.bias_ref is not None and ctx.needs_input_grad[2]
            dw, db = ops.conv_kxk_wgrad(x, gy, weight.shape[2], ctx.stride, want_bias=want_b, dw_out=grad_out(weight),
                                        db_out=grad_out(ctx.bias_ref) if want_b else None)
        return dx, dw, db, None


def conv3x3(x, weight, bias, cache, stride=1, act=ops.ACT_NONE, relu_in=False, relu_grad_by_consumer=False, precision=None):
    return Conv3x3Fn.apply(x, weight, bias, cache, stride, act, relu_in, relu_grad_by_consumer, precision)


# ------------------------------------------------------------------------------------------------
# the upsampler's tail: conv C -> 4C, PixelShuffle(2), conv C -> 3            reference model/basic.py:56-60
# ------------------------------------------------------------------------------------------------
class UpsampleTailFn(Function):
    """y = conv(pixel_shuffle(conv(h, W2) + b2), W4) + b4 as ONE node.  The forward is the two launches the two Conv3x3Fn nodes make
    (same packs, same order: the same bits), but the [N, 2H, 2W, C] tensor between them is not kept.  The gradient that arrives has 3
    channels, and nothing non-linear sits in the pair: per pixel of h the 4C-channel gradient the two big backward launches of the
    un-fused nodes consume is a linear image of a 4 x 4 window x 3 colours of it.  So the backward runs as the backward of a virtual
    3x3 conv V: C -> 64 (48 used) at h's resolution (csrc/upsample_tail.hip): gather the windows, compose V's weight, V's input and
    weight gradient on the routed conv kernels, and chain V's weight gradient back to the four parameters.  G's gradients come out in
    another, equally valid fp32 summation order."""

    @staticmethod
    def forward(ctx, h, w2, b2, w4, b4, c2: PackedConvWeights, c4: PackedConvWeights):
        h = _c(h)
        mid = _conv_fwd(h, w2, b2, c2)
        y = _conv_fwd(mid, w4, b4, c4)
        ctx.refs = (w2, b2, w4, b4)
        ctx.save_for_backward(h, w2, b2, w4)
        return y

    @staticmethod
    def backward(ctx, gy):
        h, w2, b2, w4 = ctx.saved_tensors
        p_w2, p_b2, p_w4, p_b4 = ctx.refs
        need_dh, want = ctx.needs_input_grad[0], tuple(ctx.needs_input_grad[1:5])
        gw = ops.upsample_tail_gather(_c(gy))
        dh, grads = None, (None, None, None, None)
        with ops.use_precision("fp32"):       # (the mode the forward's eligibility was decided under)
            if need_dh:
                # V's weight is made anew in every backward: its packing lives in a cache of this call's own (a cache keyed by the
                # tensor's address would take the next step's weight, composed into a recycled buffer, for this one)
                weff, cache = ops.upsample_tail_compose(w2.detach(), w4.detach()), PackedConvWeights()
                wpd = _dgrad_pack(weff, cache, h.shape, 1)
            if any(want):
                S, T = ops.conv3x3_wgrad(h, gw, 1, want_bias=True)
                outs = tuple(grad_out(p) if wnt else None for p, wnt in zip((p_w2, p_b2, p_w4, p_b4), want))
                grads = ops.upsample_tail_chain(w2.detach(), b2.detach(), w4.detach(), S, T, want, outs)
            if need_dh:
                dh = _conv_dgrad(gw, weff, cache, h.shape, wpd=wpd)
        return (dh, *grads, None, None)


def upsample_tail(h, conv2, conv4):
    """conv4(pixel_shuffle(conv2(h))) for the two last Conv modules of an Upsampler (conv2 packed with the PixelShuffle fused into its
    store): the collapsed-backward node where it applies, else the two nodes of their own."""
    if conv2.bias is not None and conv4.bias is not None and ops.upsample_tail_eligible(h, h.shape[3]):
        return UpsampleTailFn.apply(h, conv2.weight, conv2.bias, conv4.weight, conv4.bias, conv2.packed, conv4.packed)
    mid = conv3x3(h, conv2.weight, conv2.bias, conv2.packed)
    return conv3x3(mid, conv4.weight, conv4.bias, conv4.packed)


# ------------------------------------------------------------------------------------------------
# conv + residual add (body tail: `res += x`, reference model/pesr.py:32-33)
# ------------------------------------------------------------------------------------------------
class ConvAddFn(Function):
    """y = conv(x, w) + b + skip"""

    @staticmethod
    def forward(ctx, x, skip, weight, bias, cache):
        x, skip = _c(x), _c(skip)
        y = _conv_fwd(x, weight, bias, cache, skip=skip)
        ctx.cache, ctx.bias_ref = cache, bias
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = _c(gy)
        wpd = _dgrad_pack(weight, ctx.cache, x.shape, 1) if ctx.needs_input_grad[0] else None
        dw, db = _conv_wgrad(x, gy, weight, ctx.bias_ref, 1, False, ctx.needs_input_grad[2], True, where="g")
        dx = _conv_dgrad(gy, weight, ctx.cache, x.shape, wpd=wpd) if ctx.needs_input_grad[0] else None
        return dx, gy, dw, db, None


# ------------------------------------------------------------------------------------------------
# ResBlock: x + res_scale * conv2(relu(conv1(x)))             reference model/basic.py:33-52
# ------------------------------------------------------------------------------------------------
class ResBlockFn(Function):
    """Four MFMA kernels forward+backward per conv pair, no standalone elementwise pass:
    forward : r = relu(conv1(x)+b1) ; y = res_scale*(conv2(r)+b2) + x        (ReLU / scale / skip in epilogues)
    backward: dr = res_scale * dgrad2(gy) masked by r>0 ; dx = dgrad1(dr) + gy  (mask / fan-in add in epilogues)
    """

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, c1: PackedConvWeights, c2: PackedConvWeights, res_scale):
        x = _c(x)
        r = _conv_fwd(x, w1, b1, c1, act=ops.ACT_RELU)
        y = _conv_fwd(r, w2, b2, c2, alpha=res_scale, skip=x)
        ctx.c1, ctx.c2, ctx.res_scale = c1, c2, res_scale
        ctx.b1_ref, ctx.b2_ref = b1, b2
        ctx.save_for_backward(x, r, w1, w2)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, r, w1, w2 = ctx.saved_tensors
        gy = _c(gy)
        s = ctx.res_scale
        need_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[3]
        # (packing happens on the main stream, before the first weight gradient)
        wpd2, wpd1 = _dgrad_pack(w2, ctx.c2, x.shape, 1, False), _dgrad_pack(w1, ctx.c1, x.shape, 1, False)
        dw2, db2 = _conv_wgrad(r, gy, w2, ctx.b2_ref, 1, False, need_w, True, alpha=s, where="g")
        dr = _conv_dgrad(gy, w2, ctx.c2, r.shape, alpha=s, mask=r, wpd=wpd2)
        dw1, db1 = _conv_wgrad(x, dr, w1, ctx.b1_ref, 1, False, need_w, True, where="g")
        dx = _conv_dgrad(dr, w1, ctx.c1, x.shape, skip=gy, wpd=wpd1) if ctx.needs_input_grad[0] else None
        return dx, dw1, db1, dw2, db2, None, None, None


# ------------------------------------------------------------------------------------------------
# MeanShift (trainable 1x1 conv 3->3)                         reference model/basic.py:9-17
# ------------------------------------------------------------------------------------------------
class MeanShiftFn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, x_nchw, y_nchw):
        x = _c(x)
        y = ops.meanshift_fwd(x, weight.detach(), bias.detach(), x_nchw, y_nchw)
        ctx.x_nchw, ctx.y_nchw, ctx.bias_ref = x_nchw, y_nchw, bias
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        if ctx.y_nchw:  # gradient arrives in the (NCHW) layout of y; the kernel wants NHWC
            gy = gy.permute(0, 2, 3, 1)
        gy = _c(gy)
        need_dx = ctx.needs_input_grad[0]
        dx, dw, db = ops.meanshift_bwd(gy, x, weight, ctx.x_nchw, need_dx, dw_out=grad_out(weight), db_out=grad_out(ctx.bias_ref))
        if need_dx and ctx.x_nchw:
            dx = dx.permute(0, 3, 1, 2)
        return dx, dw, db, None, None


# ------------------------------------------------------------------------------------------------
# Discriminator BasicBlock: conv(no bias) -> BatchNorm2d(train) -> LeakyReLU(0.2)   reference model/basic.py:19-31
# ------------------------------------------------------------------------------------------------
class BnLink:
    """What the block that CONSUMES a BasicBlock's output needs from it (round 6): with z, the saved statistics and the affine
    parameters of the producer's BatchNorm, the consumer's input-gradient kernel writes the gradient of the producer's output already
    multiplied by lrelu'(bn(z)) and leaves the two per-channel sums of the BatchNorm backward in its epilogue (ops.conv3x3_dgrad_bn_sums):
    the producer's backward then runs no reduction pass over the tensor.  The forward fills z .. slope; the consumer's backward fills
    part / g_ptr; the producer's backward uses them once and clears them.  Only ever attached between two blocks whose connecting tensor
    nobody else sees (Discriminator.forward's chain), so the gradient that arrives IS the tensor the consumer wrote (checked by address)."""
    __slots__ = ("z", "stats", "gamma", "beta", "slope", "part", "g_ptr")

    def __init__(self):
        self.z = self.stats = self.gamma = self.beta = self.part = self.g_ptr = None
        self.slope = 0.0


def _conv_bn_fwd(x, weight, bias, gamma, beta, running_mean, running_var, num_batches, cache, stride, eps, momentum, slope, y_nchw, training):
    """(z, y, stats) of conv -> BatchNorm -> activation, by the first route that covers the problem."""
    if not training:        # running statistics
        z = _conv_fwd(x, weight, bias, cache, stride)
        stats = ops.bn_eval_stats(running_mean, running_var, eps)
        return z, ops.bn_lrelu_eval_fwd(z, gamma, beta, stats, slope, y_nchw), stats
    bn = (gamma, beta, running_mean, running_var, num_batches, eps, momentum, slope, y_nchw)
    if bias is None and tuple(weight.shape[2:]) == (3, 3) and ops.conv_rgb_bn_eligible(x.shape[3], weight.shape[0], stride):
        # the Discriminator's features.0: the statistics come out of the conv kernel's epilogue (no pass over z for them)
        return ops.conv_rgb_bn_lrelu_fwd(x, weight.detach(), *bn)
    res = ops.conv3x3_fwd_bn_stats(x, cache.for_fwd(weight, x.shape, stride), None if bias is None else bias.detach(), weight.shape[0], stride)
    if res is not None:     # the sums came out of the conv kernel's epilogue: finalize + apply
        return (res[0], *ops.bn_finalize_apply(*res, *bn))
    z = _conv_fwd(x, weight, bias, cache, stride)
    return (z, *ops.bn_lrelu_fwd(z, *bn))


class ConvBnLReluFn(Function):
    """conv (bias optional) -> BatchNorm2d -> activation given by its negative slope (0.2 LeakyReLU, 0 ReLU, 1 none).
    training = True: batch statistics (and the running-stat update) - the Discriminator's only use; training = False: the
    running statistics (nn.BatchNorm2d in .eval(): a constructor branch of reference model/basic.py:26-30 the reference's own
    scripts never take).
    Round 6: where the conv kernel can leave the BatchNorm's sums in its epilogue (ops.conv3x3_fwd_bn_stats: the direct stride-2
    layers and the F(4,3) layers without split-K) the forward runs conv -> finalize -> apply, and the backward takes the sums of
    its reduction pass from the kernel that produced its incoming gradient (BnLink)."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, running_mean, running_var, num_batches, cache, stride, eps, momentum,
                slope, y_nchw, training, prev_link=None, link=None):
        x = _c(x)
        ctx.prev_link, ctx.link = prev_link, None
        z, y, stats = _conv_bn_fwd(x, weight, bias, gamma.detach(), beta.detach(), running_mean, running_var, num_batches, cache, stride, eps,
                                   momentum, slope, y_nchw, training)
        if link is not None and training and not y_nchw:
            link.z, link.stats, link.gamma, link.beta, link.slope = z, stats, gamma.detach(), beta.detach(), slope
            ctx.link = link
        ctx.cache, ctx.stride, ctx.slope, ctx.y_nchw, ctx.training, ctx.bias_ref = cache, stride, slope, y_nchw, training, bias
        ctx.save_for_backward(x, z, weight, gamma, beta, stats)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, z, weight, gamma, beta, stats = ctx.saved_tensors
        gy = _c(gy)
        need_p = ctx.needs_input_grad[3] or ctx.needs_input_grad[4]
        # the gradient that arrives was written by the consumer's input-gradient kernel, already multiplied by lrelu'(bn(z)), and that
        # kernel left the two sums of the BatchNorm backward (BnLink): no reduction pass
        link, part = ctx.link, None
        if link is not None and link.part is not None:
            if gy.data_ptr() != link.g_ptr or tuple(gy.shape) != tuple(z.shape):
                raise RuntimeError("pesr_amd: the masked gradient a fused input-gradient kernel wrote for this BatchNorm did not arrive as "
                                   "written (its block's output has another consumer?)")
            part, link.part, link.g_ptr = link.part, None, None
        # second use of this block inside one backward pass: the parameter gradients are ADDED to the slices the first use wrote
        # (autograd's fan-in add_ plus the copy of the sum into the flat buffer were two launches per parameter tensor); in-place
        # accumulation assumes every weight gradient is written on one stream
        again = _second_use((gamma, beta, weight), ctx.training and need_p and ctx.needs_input_grad[1] and ctx.bias_ref is None and _SIDE_OFF,
                            (gamma, beta, weight))
        bn = (z, gy, gamma.detach(), beta.detach(), stats, ctx.slope, ctx.y_nchw)
        if again:
            dz, _, _ = ops.bn_lrelu_backward(*bn, True, again[0], again[1], accumulate=True, training=ctx.training, part=part)
            dgamma = dbeta = None
        else:
            dz, dgamma, dbeta = ops.bn_lrelu_backward(*bn, need_p, grad_out(gamma) if need_p else None, grad_out(beta) if need_p else None,
                                                      training=ctx.training, part=part)
        need_dx = ctx.needs_input_grad[0]
        wpd = _dgrad_pack(weight, ctx.cache, x.shape, ctx.stride) if need_dx else None
        dw, db = _conv_wgrad(x, dz, weight, ctx.bias_ref, ctx.stride, ctx.cache.ps, ctx.needs_input_grad[1],
                             ctx.bias_ref is not None and ctx.needs_input_grad[2], where="d", again=(again[2], None) if again else None)
        dx = _conv_dgrad(dz, weight, ctx.cache, x.shape, ctx.stride, prev_link=ctx.prev_link, wpd=wpd) if need_dx else None
        return dx, dw, db, dgamma, dbeta, None, None, None, None, None, None, None, None, None, None, None, None


# ------------------------------------------------------------------------------------------------
# spectral normalisation of a conv weight (reference model/basic.py:25; torch.nn.utils.spectral_norm semantics)
# ------------------------------------------------------------------------------------------------
_SN_STAMP = [0]


class SpectralNormFn(Function):
    """w_hat = w / sigma(w), sigma = u^T W v after (in training mode) one power iteration that rewrites the u / v buffers in
    place.  backward: dw = (g - <g, w_hat> u v^T) / sigma with that forward's u, v (constants, as in torch)."""

    @staticmethod
    def forward(ctx, weight, u, v, update, eps):
        w_hat, sigma = ops.spectral_norm_fwd(_c(weight.detach()), u, v, update, eps)
        # (clones: the next forward's power iteration rewrites the buffers - torch clones them for the same reason, so that
        # loss = D(real) - D(fake) can back-propagate through two forward passes)
        ctx.save_for_backward(w_hat, u.clone(), v.clone(), sigma)
        ctx.weight_ref = weight
        return w_hat

    @staticmethod
    def backward(ctx, g):
        w_hat, u, v, sigma = ctx.saved_tensors
        return ops.spectral_norm_bwd(_c(g), w_hat, u, v, sigma, dw_out=grad_out(ctx.weight_ref)), None, None, None, None


def spectral_normalize(weight, u, v, training, eps=1e-12):
    """The normalised weight of a spectral_norm-wrapped conv for THIS forward.  It is a fresh tensor every time; a unique
    (negative) epoch keeps the packed-weight caches from mistaking it for an earlier one whose memory the allocator re-used."""
    w_hat = SpectralNormFn.apply(weight, u, v, bool(training), eps)
    _SN_STAMP[0] += 1
    setattr(w_hat, _EPOCH_ATTR, -_SN_STAMP[0])
    return w_hat


class ScaleAddFn(Function):
    """y = alpha * a + b (`res = body(x).mul(res_scale); res += x`, reference model/basic.py:49-50) - only the un-fused
    ResBlock variants need it; the default ResBlock has it in its second conv's epilogue."""

    @staticmethod
    def forward(ctx, a, b, alpha):
        ctx.alpha = alpha
        return ops.relu_mask(_c(a), None, _c(b), alpha=alpha)

    @staticmethod
    def backward(ctx, gy):
        gy = _c(gy)
        return ops.relu_mask(gy, None, None, alpha=ctx.alpha), gy, None


class ChannelAttentionFn(Function):
    """y = x + res_scale * t * s, s = sigmoid(W2 relu(W1 mean_pixels(t) + B1) + B2): the tail of a residual channel-attention block
    (docs/modes.md section 4u), t the output of the block's second conv.  Saves t and the gate's small tensors (s, h, m); x is not
    needed in backward: gx = gy.  fp32 kernels whatever ops.PRECISION is."""

    @staticmethod
    def forward(ctx, x, t, w1, b1, w2, b2, res_scale):
        x, t = _c(x), _c(t)
        m = ops.ca_pool(t)
        h, s = ops.ca_gate_fwd(m, w1.detach(), b1.detach(), w2.detach(), b2.detach())
        ctx.res_scale = res_scale
        ctx.b1_ref, ctx.b2_ref = b1, b2
        ctx.save_for_backward(t, s, h, m, w1, w2)
        return ops.ca_apply_fwd(x, t, s, res_scale)

    @staticmethod
    def backward(ctx, gy):
        t, s, h, m, w1, w2 = ctx.saved_tensors
        gy = _c(gy)
        ds = ops.ca_ds(gy, t, ctx.res_scale)
        dm, dw1, db1, dw2, db2 = ops.ca_gate_bwd(ds, s, h, m, w1, w2, grad_out(w1), grad_out(ctx.b1_ref), grad_out(w2),
                                                 grad_out(ctx.b2_ref))
        gt = ops.ca_apply_bwd(gy, s, dm, ctx.res_scale) if ctx.needs_input_grad[1] else None
        return (gy if ctx.needs_input_grad[0] else None), gt, dw1, db1, dw2, db2, None


class WindowAttentionFn(Function):
    """out = softmax(q k^T / sqrt(32)) v per 8 x 8 window and head of 32 channels (docs/modes.md section 4w); qkv: NHWC [N, H, W, 3 D].
    Saves qkv alone: the backward recomputes the attention matrix.  fp32 kernels whatever ops.PRECISION is."""

    @staticmethod
    def forward(ctx, qkv, shift):
        qkv = _c(qkv)
        ctx.shift = shift
        ctx.save_for_backward(qkv)
        return ops.window_attention_fwd(qkv, shift)

    @staticmethod
    def backward(ctx, gout):
        qkv, = ctx.saved_tensors
        return ops.window_attention_bwd(qkv, _c(gout), ctx.shift), None


class LayerNormFn(Function):
    """y = (x - mean) * rstd * gamma + beta over the channels of each pixel of an NHWC map (docs/modes.md section 4x), centred variance,
    eps = ops.LN_EPS.  Saves x, gamma and the [P, 2] (mean, rstd) the forward leaves.  fp32 kernels whatever ops.PRECISION is."""

    @staticmethod
    def forward(ctx, x, gamma, beta):
        x = _c(x)
        y, stats = ops.layernorm_fwd(x, gamma.detach(), beta.detach())
        ctx.beta_ref = beta
        ctx.save_for_backward(x, gamma, stats)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, stats = ctx.saved_tensors
        dx, dgamma, dbeta = ops.layernorm_bwd(x, gamma.detach(), stats, _c(gy), grad_out(gamma), grad_out(ctx.beta_ref))
        return (dx if ctx.needs_input_grad[0] else None), dgamma, dbeta


class BilinearUp2Fn(Function):
    """y = up2(a + b), b optional: bilinear x2 (F.interpolate(scale_factor=2, mode='bilinear', align_corners=False)) of an NHWC map, the
    decoder step of the U-Net discriminator with the skip addition in front of it folded in (docs/modes.md section 4v).  up2 is linear:
    the backward is its adjoint, one kernel, and the one tensor is the gradient of both addends.  fp32 whatever ops.PRECISION is."""

    @staticmethod
    def forward(ctx, a, b=None):
        return ops.bilinear_up2_fwd(_c(a), None if b is None else _c(b))

    @staticmethod
    def backward(ctx, gy):
        need_a, need_b = ctx.needs_input_grad[0], len(ctx.needs_input_grad) > 1 and ctx.needs_input_grad[1]
        if not (need_a or need_b):
            return None, None
        gx = ops.bilinear_up2_bwd(_c(gy))
        return (gx if need_a else None), (gx if need_b else None)


# ------------------------------------------------------------------------------------------------
# Twice-differentiable building blocks of the Discriminator (gradient penalty, reference train.py:216-226:
# torch.autograd.grad(D(x_both), x_both, create_graph=True) and then .backward() through that gradient).
# Every first-order backward here is itself an autograd Function, so the graph of dD/dx exists; the second-order
# rules are: conv dgrad <-> conv forward / wgrad, Linear likewise, LeakyReLU masks are piecewise constant, and the
# training-mode BatchNorm backward has its own backward kernel (pesr_bn_bwd_bwd).  Un-fused on purpose: autograd has
# to see z between conv and BatchNorm.  Used only for the penalty's extra D forward (Discriminator.forward_second_order).
# ------------------------------------------------------------------------------------------------
class Conv2Fn(Function):
    """z = conv(x, w), no bias."""

    @staticmethod
    def forward(ctx, x, weight, cache, stride):
        x = _c(x)
        z = _conv_fwd(x, weight, None, cache, stride)
        ctx.cache, ctx.stride = cache, stride
        ctx.save_for_backward(x, weight)
        return z

    @staticmethod
    def backward(ctx, gz):
        x, weight = ctx.saved_tensors
        gz = _c(gz)
        dx = ConvDgrad2Fn.apply(gz, weight, tuple(x.shape), ctx.cache, ctx.stride) if ctx.needs_input_grad[0] else None
        dw, _ = _conv_wgrad(x.detach(), gz.detach(), weight.detach(), None, ctx.stride, False, ctx.needs_input_grad[1], False)
        return dx, dw, None, None


class ConvDgrad2Fn(Function):
    """dx = conv_transpose(gz, w): the input gradient of Conv2Fn as a differentiable op.  Its backward for g = dL/d(dx):
    dL/d(gz) = conv(g, w) (the forward conv), dL/dw = wgrad(x := g, dy := gz)."""

    @staticmethod
    def forward(ctx, gz, weight, x_shape, cache, stride):
        gz = _c(gz)
        # (always on the packed weights: its backward differentiates that kernel's arithmetic)
        dx = _conv_dgrad(gz, weight, cache, x_shape, stride, wpd=cache.for_dgrad(weight, x_shape, stride))
        ctx.cache, ctx.stride = cache, stride
        ctx.save_for_backward(gz, weight)
        return dx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        gz, weight = ctx.saved_tensors
        g = _c(g)
        l_gz = _conv_fwd(g, weight, None, ctx.cache, ctx.stride) if ctx.needs_input_grad[0] else None
        l_w, _ = _conv_wgrad(g, gz, weight.detach(), None, ctx.stride, False, ctx.needs_input_grad[1], False)
        return l_gz, l_w, None, None, None


class Bn2Fn(Function):
    """u = gamma * xhat(z) + beta with batch statistics (nn.BatchNorm2d in training mode, running stats updated)."""

    @staticmethod
    def forward(ctx, z, gamma, beta, running_mean, running_var, num_batches, eps, momentum):
        z = _c(z)
        u, stats = ops.bn_lrelu_fwd(z, gamma.detach(), beta.detach(), running_mean, running_var, num_batches, eps, momentum, 1.0, False)
        ctx.save_for_backward(z, gamma, stats)
        return u

    @staticmethod
    def backward(ctx, gu):
        z, gamma, stats = ctx.saved_tensors
        gu = _c(gu)
        dz = dgamma = dbeta = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dz_plain, dgamma, dbeta = ops.bn_lrelu_bwd(z.detach(), gu.detach(), gamma.detach(), gamma.detach(), stats, 1.0, False, True)
        if ctx.needs_input_grad[0]:
            dz = BnBwd2Fn.apply(gu, z, gamma, stats)
        return dz, dgamma, dbeta, None, None, None, None, None


class BnBwd2Fn(Function):
    """dz = gamma * invstd * (du - mean(du) - xhat * mean(du * xhat)): the training-mode BatchNorm backward as a differentiable
    op (in du, z AND gamma: xhat and invstd depend on z)."""

    @staticmethod
    def forward(ctx, du, z, gamma, stats):
        du = _c(du)
        dz, _, _ = ops.bn_lrelu_bwd(z.detach(), du, gamma.detach(), gamma.detach(), stats, 1.0, False, False)
        ctx.save_for_backward(du, z, gamma, stats)
        return dz

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        du, z, gamma, stats = ctx.saved_tensors
        l_du, l_z, l_ga = ops.bn_bwd_bwd(z, du, _c(g), gamma, stats, ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        return l_du, l_z, l_ga, None


class LRelu2Fn(Function):
    """y = leaky_relu(u); its backward is the (differentiable) mask multiply."""

    @staticmethod
    def forward(ctx, u, slope):
        u = _c(u)
        y = ops.relu_mask(u, u, slope=slope)
        ctx.slope = slope
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        return MaskMul2Fn.apply(gy, y, ctx.slope), None


class MaskMul2Fn(Function):
    """out = gy where ref > 0, slope * gy elsewhere: linear in gy, piecewise constant in ref."""

    @staticmethod
    def forward(ctx, gy, ref, slope):
        ctx.slope = slope
        ctx.save_for_backward(ref)
        return ops.relu_mask(_c(gy), ref, slope=slope)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (ref,) = ctx.saved_tensors
        return ops.relu_mask(_c(g), ref, slope=ctx.slope), None, None


class Linear2Fn(Function):
    """y = x W^T + b."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x = _c(x)
        ctx.save_for_backward(x, weight)
        return ops.linear_fwd(x, weight.detach(), bias.detach(), ops.ACT_NONE, 0.0)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = _c(gy)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = LinDgrad2Fn.apply(gy, weight)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, db = ops.linear_wgrad(gy.detach(), x.detach(), want_bias=True)
        return dx, dw, db


class LinDgrad2Fn(Function):
    """dx = gy W; backward for g = dL/d(dx): dL/d(gy) = g W^T, dL/dW = gy^T g."""

    @staticmethod
    def forward(ctx, gy, weight):
        gy = _c(gy)
        ctx.save_for_backward(gy, weight)
        return ops.linear_dgrad(gy, weight.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        gy, weight = ctx.saved_tensors
        g = _c(g)
        l_gy = ops.linear_fwd(g, weight.detach(), None, ops.ACT_NONE, 0.0) if ctx.needs_input_grad[0] else None
        l_w = ops.linear_wgrad(gy, g, want_bias=False)[0] if ctx.needs_input_grad[1] else None
        return l_gy, l_w


# ------------------------------------------------------------------------------------------------
# Linear (+LeakyReLU)                                          reference model/pesr.py:69-74
# ------------------------------------------------------------------------------------------------
# LinearFn's second use inside one backward pass may accumulate into the flat-gradient slice in place (below).  That is only
# correct while NOTHING ELSE contributes to the same weight in that pass: a third contribution arriving as an ordinary tensor
# (the gradient penalty's LinDgrad2Fn, reference train.py:216-226) makes autograd's input buffer a fresh temporary, and an
# in-place add into the slice would then miss it - whether it does depends on the engine's node order.  Trainer switches the
# fast path off around every backward pass that runs with the penalty.
INPLACE_SECOND_USE = True


class LinearFn(Function):
    """grad_rows (optional): only the first grad_rows rows of x need an input gradient - the Discriminator's classifier on [sr; hr] in the
    generator phase, whose hr half comes from a no_grad pass (Discriminator.classify); the other rows of the returned gradient are
    never read (torch.cat's backward hands them to an input that requires none) and stay uninitialised."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, slope, grad_rows=None):
        x = _c(x)
        y = ops.linear_fwd(x, weight.detach(), bias.detach(), act, slope)
        ctx.act, ctx.slope, ctx.bias_ref, ctx.grad_rows = act, slope, bias, grad_rows
        ctx.save_for_backward(x, weight, y if act != ops.ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, y = ctx.saved_tensors
        gy = _c(gy)
        if ctx.act != ops.ACT_NONE:
            if gy.numel() % 4 == 0:
                gy = ops.relu_mask(gy, y, slope=ctx.slope if ctx.act == ops.ACT_LRELU else 0.0)
            else:  # scalar-sized tail case
                gy = torch.where(y > 0, gy, gy * (ctx.slope if ctx.act == ops.ACT_LRELU else 0.0))
        dx = None
        if ctx.needs_input_grad[0]:
            r = ctx.grad_rows
            if r is not None and 0 < r < gy.shape[0]:
                dx = torch.empty((gy.shape[0], weight.shape[1]), dtype=torch.float32, device=gy.device)
                ops.linear_dgrad(gy[:r], weight.detach(), out=dx[:r])
            else:
                dx = ops.linear_dgrad(gy, weight.detach())
        dw = db = None
        if ctx.needs_input_grad[1]:
            o_w, o_b = grad_out(weight), grad_out(ctx.bias_ref)
            # second use of this layer in the same backward pass: accumulate straight into the slices the first use wrote and hand
            # autograd nothing to add - for classifier.0 that add was a 302 MB elementwise kernel
            again = _second_use((weight, ctx.bias_ref), o_w is None and o_b is None, (weight,))
            if again:
                ops.linear_wgrad(gy, x, want_bias=True, dw_out=again[0], db_out=again[1], accumulate=True)
                return dx, None, None, None, None, None
            dw, db = ops.linear_wgrad(gy, x, want_bias=True, dw_out=o_w, db_out=o_b)
        return dx, dw, db, None, None, None


class SplitRowsFn(Function):
    """t[:n], t[off:off + n] whose backward is ONE buffer (two slicing nodes cost two zero fills, two copies and an add - five launches
    for the [2B, 1] logits of the Discriminator's paired classifier).  Rows outside the two pieces get zero gradients."""

    @staticmethod
    def forward(ctx, t, n, off):
        ctx.n, ctx.off, ctx.rows = n, off, t.shape[0]
        return t[:n].clone(), t[off:off + n].clone()

    @staticmethod
    def backward(ctx, ga, gb):
        if ga is None and gb is None:
            return None, None, None
        ref = ga if ga is not None else gb
        if ctx.off == ctx.n and ctx.rows == 2 * ctx.n and ga is not None and gb is not None:
            return torch.cat([ga, gb]), None, None
        g = ref.new_zeros((ctx.rows,) + tuple(ref.shape[1:]))
        if ga is not None:
            g[:ctx.n] = ga
        if gb is not None:
            g[ctx.off:ctx.off + ctx.n] = gb
        return g, None, None


# ------------------------------------------------------------------------------------------------
# 2x2 max-pool behind a ReLU                                   torchvision vgg19 features (reference model/vgg.py:8-10)
# ------------------------------------------------------------------------------------------------
class MaxPoolFn(Function):
    @staticmethod
    def forward(ctx, x, relu_in):
        x = _c(x)
        if ctx.needs_input_grad[0] and (x.shape[1] % 2 or x.shape[2] % 2):
            # the forward kernel floors an odd side (the LPIPS trunk, under no_grad, relies on it); the backward does not exist for one
            raise ops._lib.PesrHipError(f"MaxPoolFn: a {x.shape[1]} x {x.shape[2]} input needs a gradient, and the max-pool backward takes "
                                        "even sides only")
        ctx.relu_in = relu_in
        ctx.save_for_backward(x)
        return ops.maxpool2x2_fwd(x)

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        return ops.maxpool2x2_bwd(x, _c(gy), ctx.relu_in), None


# ------------------------------------------------------------------------------------------------
# the LPIPS head of one tapped layer as a loss                 docs/modes.md section 4o
# ------------------------------------------------------------------------------------------------
class LpipsLayerFn(Function):
    """(fa, fb, w) -> float64 [N], ops.lpips_layer_pair; only fa gets a gradient (fb is the no_grad hr pass, the weights are frozen):
    ops.lpips_layer_bwd on the saved features.  The gradient is NOT masked by fa > 0: fa is a tap, the output of a ReLU that the next
    conv or pool consumes too, and the tap's conv masks the sum of the two gradients (Conv3x3Fn with relu_grad_by_consumer = False)."""

    @staticmethod
    def forward(ctx, fa, fb, w):
        fa, fb, w = _c(fa), _c(fb), _c(w.detach())
        ctx.save_for_backward(fa, fb, w)
        return ops.lpips_layer_pair(fa, fb, w)

    @staticmethod
    def backward(ctx, g):
        fa, fb, w = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        return ops.lpips_layer_bwd(fa, fb, w, _c(g)), None, None


def lpips_layer(fa, fb, w):
    return LpipsLayerFn.apply(fa, fb, w)


# ------------------------------------------------------------------------------------------------
# SSIM-Y on the unquantised luma as a loss                     docs/modes.md section 4p
# ------------------------------------------------------------------------------------------------
class SsimLossFn(Function):
    """(sr, hr) [N, 3, H, W] -> float64 [N], ops.ssim_loss_fwd; only sr gets a gradient: ops.ssim_loss_bwd on the saved images and the
    saved per-window coefficients.  When sr needs no gradient the coefficients are never written."""

    @staticmethod
    def forward(ctx, a, b):
        need = ctx.needs_input_grad[0]
        score, coef = ops.ssim_loss_fwd(a, b, need)
        if need:
            ctx.save_for_backward(a, b, coef)
        return score

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        a, b, coef = ctx.saved_tensors
        return ops.ssim_loss_bwd(a, b, coef, _c(g)), None


def ssim_loss(sr, hr):
    return SsimLossFn.apply(sr, hr)


# ------------------------------------------------------------------------------------------------
# texture loss of one tapped layer: patch-wise Gram matrices    docs/modes.md section 4q
# ------------------------------------------------------------------------------------------------
class TextureLayerFn(Function):
    """(fa, fb) NHWC [N, H, W, C] -> float64 [N]: ops.gram of both, ops.gram_loss; only fa gets a gradient (fb is the no_grad hr pass):
    ops.gram_bwd on the saved fa and the saved difference dG, which is never written when fa needs no gradient.  Like LpipsLayerFn's,
    the gradient is NOT masked by fa > 0: the tap's own conv masks the sum of its consumers' gradients."""

    @staticmethod
    def forward(ctx, fa, fb, patch):
        need = ctx.needs_input_grad[0]
        fa, fb = _c(fa), _c(fb)
        t, dg = ops.gram_loss(ops.gram(fa, patch), ops.gram(fb, patch), need)
        ctx.patch = patch
        if need:
            ctx.save_for_backward(fa, dg)
        return t

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        fa, dg = ctx.saved_tensors
        return ops.gram_bwd(fa, dg, _c(g), ctx.patch), None, None


def texture_layer(fa, fb, patch=0):
    return TextureLayerFn.apply(fa, fb, patch)


# ------------------------------------------------------------------------------------------------
# contextual loss of one tapped layer    docs/modes.md section 4r
# ------------------------------------------------------------------------------------------------
class ContextualLayerFn(Function):
    """(fa, fb) NHWC [N, H, W, C] -> float64 [N], -log CX: ops.cx_normalize, ops.cx_dist, ops.cx_fwd; only fa gets a gradient (fb is the
    no_grad hr pass), ops.cx_bwd on what the three stages left, with the selections held fixed.  When fa needs no gradient nothing is
    saved.  Like TextureLayerFn's, the gradient is NOT masked by fa > 0: the tap's own conv masks the sum of its consumers' gradients."""

    @staticmethod
    def forward(ctx, fa, fb, h):
        need = ctx.needs_input_grad[0]
        fa, fb = _c(fa), _c(fb)
        xh, yh, inv, _ = ops.cx_normalize(fa, fb)
        D, m, b = ops.cx_dist(xh, yh)
        L, CX, S, a, cmax = ops.cx_fwd(D, m, h, fa.shape[3])
        ctx.h, ctx.shape = float(h), tuple(fa.shape)
        if need:
            ctx.save_for_backward(xh, yh, inv, D, m, b, S, a, cmax, CX)
        return L

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        xh, yh, inv, D, m, b, S, a, cmax, CX = ctx.saved_tensors
        return ops.cx_bwd(_c(g), xh, yh, inv, D, m, b, S, a, cmax, CX, ctx.h, ctx.shape), None, None


def contextual_layer(fa, fb, h=0.5):
    return ContextualLayerFn.apply(fa, fb, h)


class VggTailFn(Function):
    """conv4_1 .. conv5_4 (+ pool4) of vgg19 features[:35] (reference model/vgg.py:8-10,19-26) for the sr AND the hr branch in one
    batch: forward on cat(a, b) - one launch per layer over 2B images instead of two over B -, backward on the sr half only (the
    hr branch is the reference's no_grad pass; the weights are frozen, so the backward is a chain of input gradients).  steps:
    [(kind, module, has_relu)] from VGG._steps.  Per layer exactly what Conv3x3Fn / MaxPoolFn do: a conv's ReLU is fused into its
    epilogue and its mask is applied by the consumer's backward (the next conv's input gradient or the pool's)."""

    @staticmethod
    def forward(ctx, a, b, steps):
        B = a.shape[0]
        x = torch.cat([_c(a), _c(b)])
        plan, saved, prev_relu = [], [], False
        for kind, m, has_relu in steps:
            saved.append(x[:B])                     # (the sr half: a contiguous view)
            if kind == "conv":
                plan.append((kind, m, prev_relu, tuple(x[:B].shape)))
                x = _conv_fwd(x, m.weight, m.bias, m.packed, act=ops.ACT_RELU if has_relu else ops.ACT_NONE)
                prev_relu = has_relu
            else:
                plan.append((kind, m, prev_relu, None))
                x = ops.maxpool2x2_fwd(x)
                prev_relu = False
        ctx.plan = plan
        ctx.save_for_backward(*saved)
        fa, fb = x[:B], x[B:]
        ctx.mark_non_differentiable(fb)
        return fa, fb

    @staticmethod
    def backward(ctx, ga, _gb):
        g = _c(ga)
        for (kind, m, relu_in, shape), xin in zip(reversed(ctx.plan), reversed(ctx.saved_tensors)):
            if kind == "conv":
                g = _conv_dgrad(g, m.weight, m.packed, shape, mask=xin if relu_in else None)
            else:
                g = ops.maxpool2x2_bwd(xin, g, relu_in)
        return g, None, None


# ------------------------------------------------------------------------------------------------
# losses                                                       reference train.py:131-140
# ------------------------------------------------------------------------------------------------
class L1LossFn(Function):
    """nn.L1Loss() (mean) on NHWC 3-channel tensors; the gradient is produced in the same pass."""

    @staticmethod
    def forward(ctx, sr, hr):
        sr, hr = _c(sr), _c(hr)
        out, grad = ops.loss_l1_tv(sr, hr, 1.0 / sr.numel(), 0.0, need_grad=sr.requires_grad)
        ctx.save_for_backward(grad)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None


class TVLossFn(Function):
    """Sum of absolute horizontal + vertical differences (reference train.py:137-140)."""

    @staticmethod
    def forward(ctx, sr):
        sr = _c(sr)
        out, grad = ops.loss_l1_tv(sr, sr, 0.0, 1.0, need_grad=sr.requires_grad)
        ctx.save_for_backward(grad)
        return out[1]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g


class MSELossFn(Function):
    """F.mse_loss(a, b) (mean); only `a` gets a gradient (b is the no_grad branch, reference model/vgg.py:24-26)."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = _c(a), _c(b)
        out, grad = ops.loss_mse(a, b, 2.0 / a.numel(), need_grad=a.requires_grad)
        ctx.save_for_backward(grad)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None


class GanLossFn(Function):
    """The discriminator (side 0) or generator (side 1) loss of reference train.py:210-213 / :244-253 on the [B, 1] logits, scaled
    (alpha_gan): one kernel computes the value and both gradients (ops.gan_loss); backward only scales them."""

    @staticmethod
    def forward(ctx, pred_real, pred_fake, gan_type, side, focal, gamma, scale):
        pr, pf = _c(pred_real), _c(pred_fake)
        # [B, 1] logits of up to 1024 samples: the one-workgroup kernel, as ever; a logit map ([B, 1, H, W], or a longer vector): the
        # map kernels (docs/modes.md section 4v)
        fn = ops.gan_loss if pr.dim() == 2 and pr.shape[1] == 1 and pr.shape[0] <= 1024 else ops.gan_loss_map
        out, d_r, d_f = fn(pr, pf, gan_type, side, focal, gamma, scale, need_real=pred_real.requires_grad,
                           need_fake=pred_fake.requires_grad)
        ctx.save_for_backward(d_r, d_f)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        d_r, d_f = ctx.saved_tensors
        return (None if d_r is None else d_r * g), (None if d_f is None else d_f * g), None, None, None, None, None


def gan_loss(pred_real, pred_fake, gan_type, side, focal=False, gamma=1.0, scale=1.0):
    return GanLossFn.apply(pred_real, pred_fake, gan_type, side, bool(focal), float(gamma), float(scale))


def l1_loss(sr, hr):
    return L1LossFn.apply(sr, hr)


def tv_loss(sr):
    return TVLossFn.apply(sr)


def mse_loss(a, b):
    return MSELossFn.apply(a, b)
