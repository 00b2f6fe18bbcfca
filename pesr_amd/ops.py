"""Tensor-level wrappers over the C ABI (no autograd here; see functional.py).

All activation tensors handled here are fp32, on a GPU, NHWC-contiguous: shape [N, H, W, C].
(The nn.Module boundary works with logical NCHW tensors in torch.channels_last memory format; a
`.permute(0, 2, 3, 1)` of those is exactly this view - no copies.)
There is no CPU path: a CPU tensor raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import NamedTuple, Optional

import torch

from . import _lib

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2


def _chk(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise _lib.PesrHipError(f"{name}: pesr_amd ops run only on a GPU (HIP) tensor; there is no CPU fallback")
    if t.dtype != torch.float32:
        raise _lib.PesrHipError(f"{name}: expected float32, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.PesrHipError(f"{name}: expected a contiguous tensor (NHWC physical layout)")


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class _Events:
    """Optional HIP-event brackets around kernel launches, recorded on the stream the kernel is launched on (torch's current stream);
    off unless enabled.  enable(shape) watches the launches whose begin() names that shape, and keeps their times per begin() key."""

    def __init__(self):
        self.shape, self.pairs, self.every, self._n = None, {}, 1, {}

    def enable(self, shape=(), every=1):
        """Watch launches of `shape`; bracket every `every`-th launch of each key (two event records per bracket are not free:
        bracketing all ~200 watched launches of a GAN step cost 2 % of the step)."""
        self.shape, self.pairs, self.every, self._n = tuple(shape), {}, max(1, int(every)), {}

    def begin(self, key, *shape):
        """-> an open bracket (or None when this launch is not the watched shape / not sampled); close it with end()."""
        if self.shape is None or self.shape != shape:
            return None
        n = self._n.get(key, 0)
        self._n[key] = n + 1
        if n % self.every:
            return None
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        return (key, e0)

    def end(self, br):
        if br is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.pairs.setdefault(br[0], []).append((br[1], e1))

    def drain(self):
        """-> {key: (average milliseconds per launch, launches)}; disables recording."""
        pairs, self.pairs, self.shape = self.pairs, {}, None
        if not pairs:
            return {}
        torch.cuda.synchronize()
        return {k: (sum(a.elapsed_time(b) for a, b in v) / len(v), len(v)) for k, v in pairs.items()}


# Every launch of ONE conv shape (N, H, W, Cin, Cout, stride), kept per kind "fwd" / "dgrad" / "wgrad": bench.py's live roofline figures.
# Not inside a captured step: an event recorded under capture is only a dependency and cannot be timed, and recording it as an
# external event node (hipEventRecordWithFlags(hipEventRecordExternal)) is refused under capture by this ROCm runtime
# (hipErrorInvalidValue; tried in round 3) - bench.py --hip-graph takes its kernel times from eager steps.
KERNEL_EVENTS = _Events()
# The HBM-bound ops that have no conv shape key, kept per op name (bench.py's config-5 side measurement: the C -> 3 and 3 -> C convs,
# MeanShift): enable() without a shape watches them all.
OP_EVENTS = _Events()


class _FlopCount:
    """Optional tally of the matrix-pipe work of a step (bench.py's step_issued_frac): per conv / Linear launch the
    ALGORITHMIC flops of the op and the flops the dispatched kernel ISSUES for them (x 1/2 on the F(4,3) kernels, x 2/3 on
    F(2,3), x 1 on the direct ones; zero padding of the direct kernels' tiles is not counted as issued work)."""

    def __init__(self):
        self.on, self.alg, self.issued, self.by = False, 0.0, 0.0, {}

    def start(self):
        self.on, self.alg, self.issued, self.by = True, 0.0, 0.0, {}

    def stop(self):
        self.on = False
        return {"algorithmic": self.alg, "issued": self.issued, "by_kernel_family": dict(self.by)}

    def add(self, flops, frac, family):
        if self.on:
            self.alg += flops
            self.issued += flops * frac
            a = self.by.setdefault(family, [0.0, 0.0])
            a[0] += flops
            a[1] += flops * frac


FLOPS = _FlopCount()


_workspaces = {}


def workspace(nbytes: int, device: torch.device) -> torch.Tensor:
    """Grow-only per-device scratch buffer (owned by torch's caching allocator)."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


_MEMO = {}


def _memo(fn: str, *args, cache=_MEMO):
    """The library's host-only planner call `fn(*args)` (a score, a row count: pure functions of their arguments), asked once."""
    key = (fn, *args)
    v = cache.get(key)
    if v is None:
        v = cache[key] = int(getattr(_lib.lib(), fn)(*args))
    return v


# ------------------------------------------------------------------------------------------------
# 3x3 conv family
# ------------------------------------------------------------------------------------------------
USE_WINO = os.environ.get("PESR_WINO", "1") != "0"     # PESR_WINO=0: direct kernel everywhere
USE_WINO4 = os.environ.get("PESR_WINO4", "1") != "0"   # PESR_WINO4=0: no F(4,3) kernel (F(2,3) / direct instead)
# PESR_WGRAD_WINO=0: direct weight-gradient kernel everywhere (passed to the library as the explicit `algo` argument)
USE_WGRAD_WINO = os.environ.get("PESR_WGRAD_WINO", "1") != "0"
USE_WGRAD_WINO4 = os.environ.get("PESR_WGRAD_WINO4", "1") != "0"   # =0: F(2,3) weight gradient instead of F(4,3)


WGRAD_AUTO, WGRAD_DIRECT, WGRAD_WINO23, WGRAD_WINO4_12W = 0, 1, 2, 5      # include/pesr_hip.h PESR_WGRAD_* (3 and 4 are retired)
# include/pesr_hip.h PESR_WGRAD_KERNEL_* (the answer of pesr_conv3x3_wgrad_kernel) -> (kernel name, fraction of the algorithmic flops it
# issues on the matrix pipe, the key FLOPS.add files them under)
_WGRAD_KERNELS = (("conv3x3_wgrad_kernel", 1.0, "direct"),
                  ("conv3x3_wgrad_wino_kernel", 2.0 / 3.0, "F(2,3)"),
                  None, None,          # 2, 3: retired, never answered any more (the rows below keep their indices)
                  ("conv3x3_wgrad_wino4x_kernel", 1.0 / 3.0, "F(2,3)y x F(4,3)x"),
                  ("conv3x3_wgrad_wino4p_kernel", 1.0 / 3.0, "F(2,3)y x F(4,3)x"))


def _wgrad_algo():
    """The `algo` argument the PESR_WGRAD_* / PESR_WINO4 switches ask for."""
    if not USE_WGRAD_WINO:
        return WGRAD_DIRECT
    if not (USE_WINO4 and USE_WGRAD_WINO4):
        return WGRAD_WINO23
    return WGRAD_AUTO


def _wgrad_kernel(N, H, W, Cin, Cout, stride, ps_in, algo, accumulate):
    """The library's own answer: the _WGRAD_KERNELS row of the kernel pesr_conv3x3_wgrad runs for these arguments (the direct kernel's
    row for a shape the call refuses)."""
    return _WGRAD_KERNELS[max(0, _memo("pesr_conv3x3_wgrad_kernel", N, H, W, Cin, Cout, stride, int(ps_in), algo, int(accumulate)))]


def _wg4_plan_ok(N, H, W, Cin, Cout):
    """wg4_plan of csrc/conv3x3_wgrad_wino4.hip, asked of the library: (covered, images per strip)."""
    side = _memo("pesr_conv3x3_wgrad_wino4_side", N, H, W, Cin, Cout)
    return side > 0, max(side, 1)


def wgrad_kernel_for(N, H, W, Cin, Cout):
    """(kernel name, fraction of the algorithmic flops it issues on the matrix pipe) of the stride-1 weight gradient, as
    conv3x3_wgrad dispatches it under the current switches (plain gradient, not accumulating)."""
    return _wgrad_kernel(N, H, W, Cin, Cout, 1, False, _wgrad_algo(), False)[:2]


def wino_eligible(N: int, H: int, W: int, Cin: int, Cout: int, stride: int = 1) -> bool:
    """The Winograd kernel applies (stride 1, even width, Cout % 128 == 0) AND its 288-pixel x 128-channel tiles fill the
    chip; small layers stay on the direct kernel (smaller tiles, split-K).  Cin / Cout are those of the problem the kernel
    runs (for an input gradient: Cin = the forward conv's Cout and vice versa)."""
    if not USE_WINO or stride != 1 or W % 2 or Cin % 64 or Cout % 128:
        return False
    per_img = (H * (W // 2) + 143) // 144
    wgs = N * per_img * (Cout // 128)
    if wgs >= 192:
        return True
    # fewer tiles: the kernel splits the Cin chunks over up to Cin/64 workgroups per tile - worth it while the 144-x-tile
    # tiles are (nearly) full, i.e. from 24x24 images up
    return per_img * 144 <= 1.15 * H * (W // 2) and wgs * min(8, Cin // 64) >= 192


def wino4_eligible(N: int, H: int, W: int, Cin: int, Cout: int, stride: int = 1, ps_out: bool = False) -> bool:
    """The F(4,3) kernel applies (stride 1, W % 4 == 0, Cin % 16 == 0, Cout % 64 == 0; Cout % 256 == 0 with a fused
    PixelShuffle store), its 576-pixel x 64-channel tiles (split-K included) give at least 192 workgroups, AND at least 78 %
    of the tile area lies inside the image: it issues 1/2 of the direct conv's MFMAs where F(2,3) issues 2/3, so it wins
    from ~0.75 of F(2,3)'s tile efficiency up.  Cin / Cout are those of the problem the kernel runs."""
    if not (USE_WINO and USE_WINO4) or stride != 1 or W % 4 or Cin % 16 or Cout % 64 or (ps_out and Cout % 256):
        return False
    return _memo("pesr_conv3x3_wino4_score", N, H, W, Cin, Cout, 0 if ps_out else 1) >= 780


# ---- the OPTIONAL bf16-operand mode --------------------------------------------------------------------------------
# PRECISION = "bf16" (set_precision / PESR_PRECISION / train.py --precision): the stride-1 convs with 32-multiple input and
# 64-multiple output channels run on v_mfma_f32_16x16x32_bf16 - operands rounded to bf16, fp32 accumulation, fp32 tensors in HBM.
# Everything else (and everything by default) stays on the fp32 kernels.
PRECISION = os.environ.get("PESR_PRECISION", "fp32")
_BF16_NO_S2 = os.environ.get("PESR_BF16_NO_S2", "0") == "1"      # A/B switch of scripts/gpu_call51.sh: stride-2 forwards stay fp32
# layers whose bf16 launch would have fewer workgroups stay on the fp32 kernels (tests lower it; at 64 workgroups the 16x12x12x512
# layers take 47 us against 89 on the F(4,3) kernel, scripts/bf16_small_time.py).  The env form is for A/B runs only.
BF16_MIN_WGS = int(os.environ.get("PESR_BF16_MIN_WGS", "64"))
PRECISIONS = ("fp32", "bf16", "split-bf16")


def set_precision(p: str) -> None:
    global PRECISION
    if p not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}, got {p!r}")
    PRECISION = p


class use_precision:
    """with use_precision(p): PRECISION is p inside and what it was outside; p = None changes nothing.  For a node whose kernels must not
    depend on the mode that happens to be set when it runs (the LPIPS trunk's input gradients, docs/modes.md section 4o)."""

    def __init__(self, p: Optional[str]):
        if p is not None and p not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}, got {p!r}")
        self.p, self.prev = p, None

    def __enter__(self):
        global PRECISION
        self.prev = PRECISION
        if self.p is not None:
            PRECISION = self.p

    def __exit__(self, *a):
        global PRECISION
        PRECISION = self.prev


def bf16_eligible(N: int, H: int, W: int, Cin: int, Cout: int, stride: int = 1, ps_out: bool = False, ps_in: bool = False) -> bool:
    """PRECISION is "bf16" and the bf16 kernel covers the shape with at least 78 % of its tile area inside the image.
    Cin / Cout are those of the problem the kernel runs."""
    bn = 256 if Cout % 256 == 0 else (128 if Cout % 128 == 0 else 64)        # output channels per workgroup (conv3x3_bf16.hip)
    if PRECISION != "bf16" or stride not in (1, 2) or Cin % 32 or Cout % 64 or (ps_out and Cout % (4 * bn)) or (ps_in and Cin % 128):
        return False
    if stride == 2 and (ps_out or ps_in or _BF16_NO_S2):
        return False
    # stride 2: the FORWARD kernel only (H, W: the input's size); its gradients stay on the fp32 kernels
    return _memo("pesr_conv3x3_bf16_score" if stride == 1 else "pesr_conv3x3_bf16_s2_score", N, H, W, Cin, Cout, BF16_MIN_WGS) >= 780


def bf16_s2_dgrad_eligible(N: int, H: int, W: int, Cout_fwd: int, Cin_fwd: int) -> bool:
    """PRECISION is "bf16" and the stride-2 input-gradient form of the bf16 kernel covers dx [N, H, W, Cin_fwd]."""
    if PRECISION != "bf16" or _BF16_NO_S2 or Cout_fwd % 32 or Cin_fwd % 64:
        return False
    return _memo("pesr_conv3x3_bf16_s2_dgrad_score", N, H, W, Cout_fwd, Cin_fwd, BF16_MIN_WGS) >= 780


# ---- the OPTIONAL split-bf16 mode (round 4) ---------------------------------------------------------------------------
# PRECISION = "split-bf16": forward and input gradient of the stride-1 convs with Cin % 32 == 0 and Cout % 128 == 0 run on the bf16
# MFMA with every operand split into hi + lo bf16 terms and three products per multiply (conv3x3_bf16x3.hip): 3.6 .. 4.7e-6 of the
# output maximum against fp64 - inside the fp32 kernels' own tolerances, so the mode is tested against the fp32 oracle.  Weight
# gradients, stride-2 convs, 64-channel layers and everything else stay on the fp32 kernels.
BF16X3_MIN_WGS = 128


def bf16x3_eligible(N: int, H: int, W: int, Cin: int, Cout: int, stride: int = 1, ps_out: bool = False, ps_in: bool = False) -> bool:
    """PRECISION is "split-bf16" and the split kernel covers the problem it would run (an input gradient: Cin / Cout swapped)."""
    # (ps_out: an n-tile - 256 or 128 channels, the planner's choice - must stay inside one of the four sub-pixel planes)
    if PRECISION != "split-bf16" or stride != 1 or Cin % 32 or Cout % 128 or (ps_out and Cout % 1024) or (ps_in and Cin % 128):
        return False
    return _memo("pesr_conv3x3_bf16x3_score", N, H, W, Cin, Cout, BF16X3_MIN_WGS) >= 780


# ---- the kernel families: one record each.  Packing, the batched re-pack's mode numbers, the flop tally, the launch and the dispatch
# priority (here and in functional.PackedConvWeights) all read this table. ---------------------------------------------------------
class _Packed:
    """Weights packed for one of the kernel families below: the buffer `.t` and, per subclass, its `.family` record.  (The direct
    kernels' packing is a bare tensor.)  conv3x3_fwd / conv3x3_dgrad dispatch on it."""
    __slots__ = ("t",)

    def __init__(self, t: torch.Tensor):
        self.t = t

    def data_ptr(self) -> int:      # (as the bare tensor of the direct packing has it)
        return self.t.data_ptr()


class WinoPacked(_Packed):
    """Weights packed for the Winograd F(2,3)-along-x kernel (pesr_pack_conv3x3_wino)."""
    __slots__ = ()


class Wino4Packed(_Packed):
    """Weights packed for the Winograd F(4,3)-along-x kernel (pesr_pack_conv3x3_wino4)."""
    __slots__ = ()


class Bf16Packed(_Packed):
    """Weights rounded to bf16 and packed for conv3x3_bf16_kernel (pesr_pack_conv3x3_bf16)."""
    __slots__ = ()


class Bf16x3Packed(_Packed):
    """Weights split into hi + lo bf16 planes and packed for conv3x3_bf16x3_kernel (pesr_pack_conv3x3_bf16x3)."""
    __slots__ = ()


class _Family(NamedTuple):
    name: str                   # as the dispatch tests and documents call it
    mode: int                   # mode number of its forward packing in the batched re-pack (csrc/pack.hip); the dgrad packing is mode + 1
    wrap: Optional[type]        # class of its packed weights; None: a bare tensor
    pack: str                   # C entry point of the single pack
    planes: int                 # packed elements per (reduction channel, "n" channel) pair
    dtype: torch.dtype          # ... and their type
    frac: float                 # flops issued on the matrix pipe per algorithmic flop ...
    label: str                  # ... and the key FLOPS.add files them under
    launch: Optional[str]       # C entry point _conv3x3_wino launches; None: conv3x3_fwd / conv3x3_dgrad launch the direct kernels themselves
    splitk: bool                # the launch takes the split-K workspace
    eligible: object            # (N, H, W, Cin, Cout, stride, ps_out, ps_in) of the problem the KERNEL would run -> it covers it and fills the chip

    def dims(self, O: int, I: int, mode: int):
        """(R, Nn): reduction and "n" channels of the packing, mode 0 forward / 1 dgrad.  The direct kernels' packing zero-pads R to
        a multiple of 16 and Nn to 16 (if <= 16) or a multiple of 64, so the 3-channel RGB layers run on the same MFMA kernels."""
        R, Nn = (I, O) if mode == 0 else (O, I)
        if self.wrap is None:
            R, Nn = (R + 15) // 16 * 16, 16 if Nn <= 16 else (Nn + 63) // 64 * 64
        return R, Nn


# In dispatch priority: the first family that is eligible runs.
_FAMILIES = (
    _Family("split-bf16", 9, Bf16x3Packed, "pesr_pack_conv3x3_bf16x3", 18, torch.bfloat16, 3.0, "split-bf16 (3 bf16 products per multiply)",
            "pesr_conv3x3_bf16x3", False, bf16x3_eligible),
    _Family("bf16", 7, Bf16Packed, "pesr_pack_conv3x3_bf16", 9, torch.bfloat16, 1.0, "bf16",
            "pesr_conv3x3_bf16", False, bf16_eligible),
    _Family("F(4,3)", 4, Wino4Packed, "pesr_pack_conv3x3_wino4", 18, torch.float32, 0.5, "F(4,3)",
            "pesr_conv3x3_wino4", True, lambda N, H, W, Cin, Cout, s, po, pi: wino4_eligible(N, H, W, Cin, Cout, s, po)),
    _Family("F(2,3)", 2, WinoPacked, "pesr_pack_conv3x3_wino", 12, torch.float32, 2.0 / 3.0, "F(2,3)",
            "pesr_conv3x3_wino", True, lambda N, H, W, Cin, Cout, s, po, pi: wino_eligible(N, H, W, Cin, Cout, s)),
    _Family("direct", 0, None, "pesr_pack_conv3x3", 9, torch.float32, 1.0, "direct",
            None, True, lambda N, H, W, Cin, Cout, s, po, pi: True),
)
_BF16X3, _BF16, _WINO4, _WINO, _DIRECT = _FAMILIES
for _f in _FAMILIES[:-1]:
    _f.wrap.family = _f


def _conv_family(wp) -> _Family:
    return getattr(wp, "family", _DIRECT)


def conv3x3_family_fwd(N: int, H: int, W: int, Cin: int, Cout: int, stride: int, ps: bool) -> _Family:
    """The family that runs y = conv(x [N, H, W, Cin], w [Cout, Cin, 3, 3]); ps: with the PixelShuffle fused into its store."""
    for f in _FAMILIES:
        if f.eligible(N, H, W, Cin, Cout, stride, ps, False):
            return f


def conv3x3_family_dgrad(N: int, H: int, W: int, Cin: int, Cout: int, stride: int, ps: bool) -> _Family:
    """The family that runs dx [N, H, W, Cin] of that conv: the stride-1 kernels on the problem with Cin and Cout swapped.  At stride 2
    only the bf16 kernel has an input-gradient form besides the direct one (on the bf16 dgrad packing; none with a fused pixel-unshuffle)."""
    if stride != 1:
        return _BF16 if stride == 2 and not ps and bf16_s2_dgrad_eligible(N, H, W, Cout, Cin) else _DIRECT
    for f in _FAMILIES:
        if f.eligible(N, H, W, Cout, Cin, 1, False, ps):
            return f


def _pack(f: _Family, w: torch.Tensor, mode: int, ps: bool):
    """OIHW [O, I, 3, 3] fp32 -> family f's packing (mode 0: forward, mode 1: dgrad; ps: sub-pixel-major O order)."""
    name = f.pack[len("pesr_"):]
    _chk(w, f"{name}.w")
    O, I = w.shape[0], w.shape[1]
    assert tuple(w.shape[2:]) == (3, 3), f"{name}: a 3x3 kernel is required, got {tuple(w.shape)}"
    R, Nn = f.dims(O, I, mode)
    out = torch.empty(f.planes * R * Nn, dtype=f.dtype, device=w.device)
    rc = getattr(_lib.lib(), f.pack)(_p(w), _p(out), O, I, mode, int(ps), _stream())
    _lib.check(rc, f.pack if f.wrap is None else f"{f.pack}[{O}x{I},mode{mode}]")
    return out if f.wrap is None else f.wrap(out)


def pack_conv3x3(w: torch.Tensor, mode: int, ps: bool = False) -> torch.Tensor:
    """OIHW [O, I, 3, 3] -> packed [9, R/16, Nn, 16] (mode 0: forward, mode 1: dgrad)."""
    return _pack(_DIRECT, w, mode, ps)


def pack_conv3x3_wino(w: torch.Tensor, mode: int, ps: bool = False) -> WinoPacked:
    """OIHW [O, I, 3, 3] -> transformed [12, R/16, Nn, 16] (mode 0: forward, mode 1: dgrad; ps: sub-pixel-major O order)."""
    return _pack(_WINO, w, mode, ps)


def pack_conv3x3_wino4(w: torch.Tensor, mode: int, ps: bool = False) -> Wino4Packed:
    """OIHW [O, I, 3, 3] -> transformed [18, R/16, Nn, 16] (mode 0: forward, mode 1: dgrad; ps: sub-pixel-major O order)."""
    return _pack(_WINO4, w, mode, ps)


def pack_conv3x3_bf16(w: torch.Tensor, mode: int, ps: bool = False) -> Bf16Packed:
    """OIHW [O, I, 3, 3] fp32 -> [9, R/32, Nn, 32] bf16 (mode 0: forward, mode 1: dgrad with flipped taps; ps: sub-pixel-major O)."""
    return _pack(_BF16, w, mode, ps)


def pack_conv3x3_bf16x3(w: torch.Tensor, mode: int, ps: bool = False) -> Bf16x3Packed:
    """OIHW [O, I, 3, 3] fp32 -> [2 (hi, lo)][9, R/32, Nn, 32] bf16 (mode 0: forward, mode 1: dgrad with flipped taps; ps: sub-pixel-major O)."""
    return _pack(_BF16X3, w, mode, ps)


def pack_bias_ps(b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(b, "pack_bias_ps.b")
    if out is None:
        out = torch.empty_like(b)
    assert out.shape == b.shape and out.is_contiguous()
    _lib.check(_lib.lib().pesr_pack_bias_ps(_p(b), _p(out), b.numel(), _stream()), "pesr_pack_bias_ps")
    return out


def _conv3x3_wino(x, wp, bias, skip, mask, y, N, H, W, Cin, cout, alpha, act, slope, what, ps_out=False, ps_in=False):
    """Every family that is not the direct one (wp.family says which kernel): same arguments, same fused epilogue; the Winograd
    kernels also take the split-K scratch for layers with few tiles."""
    f = wp.family
    L = _lib.lib()
    ws_args = ()
    if f.splitk:
        nws = L.pesr_conv3x3_workspace_bytes(N, H, W, cout) if not ps_out else 0
        ws_args = (_p(workspace(nws, x.device) if nws else None), nws)
    rc = getattr(L, f.launch)(_p(x), _p(wp.t), _p(bias), _p(skip), _p(mask), _p(y), N, H, W, Cin, cout, alpha, act, slope,
                              int(ps_out), int(ps_in), *ws_args, _stream())
    _lib.check(rc, f"{f.launch}[{what} {N}x{H}x{W}x{Cin}->{cout}]")


def _conv_flops(N, OH, OW, Cin, cout, fam) -> None:
    """Tally a 3x3 conv over N x OH x OW output pixels.  fam: the _Family that runs it, its (frac, label), or a callable returning them -
    asked only while the tally is on (the weight gradient's answer is a planner call)."""
    if FLOPS.on:
        frac, label = (fam.frac, fam.label) if isinstance(fam, _Family) else fam() if callable(fam) else fam
        FLOPS.add(18.0 * N * OH * OW * Cin * cout, frac, label)


def _chk_epilogue(what: str, shape, skip, mask) -> None:
    """The tensors a fused epilogue adds (skip) or masks by (mask) have the shape of the kernel's output."""
    for t, n in ((skip, "skip"), (mask, "mask")):
        if t is not None:
            _chk(t, f"{what}.{n}")
            assert t.shape == shape, (t.shape, shape)


_RGB_VALU, _RGB_MFMA = (0.0, "rgb (HBM-bound, VALU)"), (1.0, "rgb (HBM-bound, MFMA)")
USE_RGB_OUT = True   # tests switch it off to compare with the implicit-GEMM kernel


def rgb_in_eligible(cin: int, cout: int, stride: int) -> bool:
    """Shapes of pesr_conv3x3_rgb_fwd (3 -> C, stride 1) and of its BatchNorm form; with cin and cout swapped, of pesr_conv3x3_rgb_dgrad
    (the input gradient of a C -> 3 conv is a 3 -> C conv of dy)."""
    return cin == 3 and stride == 1 and cout % 4 == 0 and 256 % (cout // 4) == 0


def wgrad_rgb_side(cin: int, cout: int) -> Optional[int]:
    """The `mode` of conv3x3_wgrad_rgb for a conv with a 3-channel side (0: the input, 1: the output); None: conv3x3_wgrad."""
    return 0 if cin == 3 else 1 if cout == 3 else None


def rgb_out_eligible(cin: int, cout: int, stride: int) -> bool:
    """Shapes of pesr_conv3x3_rgb_out_fwd (C -> 3, stride 1)."""
    return USE_RGB_OUT and cout == 3 and stride == 1 and cin % 64 == 0 and cin <= 512


def conv3x3_fwd(x: torch.Tensor, wp: torch.Tensor, bias: Optional[torch.Tensor], cout: int, stride: int = 1,
                alpha: float = 1.0, act: int = ACT_NONE, slope: float = 0.0, skip: Optional[torch.Tensor] = None,
                mask: Optional[torch.Tensor] = None, ps_out: bool = False,
                w_oihw: Optional[torch.Tensor] = None) -> torch.Tensor:
    """wp: packed weights (callable returning them is accepted, so the pack is skipped when the direct RGB kernel runs)."""
    _chk(x, "conv3x3_fwd.x")
    N, H, W, Cin = x.shape
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    if ps_out:
        y = torch.empty((N, 2 * OH, 2 * OW, cout // 4), dtype=torch.float32, device=x.device)
    else:
        y = torch.empty((N, OH, OW, cout), dtype=torch.float32, device=x.device)
    _chk_epilogue("conv3x3_fwd", y.shape, skip, mask)
    plain = skip is None and mask is None and not ps_out and alpha == 1.0 and w_oihw is not None
    if plain and rgb_in_eligible(Cin, cout, stride):
        # RGB input layer: dedicated HBM-bound direct kernel on the un-packed OIHW weights
        _conv_flops(N, OH, OW, Cin, cout, _RGB_VALU)
        br = OP_EVENTS.begin(f"conv_rgb_in 3->{cout}")
        rc = _lib.lib().pesr_conv3x3_rgb_fwd(_p(x), _p(w_oihw), _p(bias), _p(y), N, H, W, cout, act, slope, _stream())
        OP_EVENTS.end(br)
        _lib.check(rc, f"pesr_conv3x3_rgb_fwd[{N}x{H}x{W}x3->{cout}]")
        return y
    if plain and rgb_out_eligible(Cin, cout, stride):
        # -> RGB output layer: dedicated HBM-bound kernel on the un-packed OIHW weights (no pack, no padded MFMAs)
        _conv_flops(N, OH, OW, Cin, cout, _RGB_MFMA)
        br = OP_EVENTS.begin(f"conv_rgb_out {Cin}->3")
        rc = _lib.lib().pesr_conv3x3_rgb_out_fwd(_p(x), _p(w_oihw), _p(bias), _p(y), N, H, W, Cin, act, slope, _stream())
        OP_EVENTS.end(br)
        _lib.check(rc, f"pesr_conv3x3_rgb_out_fwd[{N}x{H}x{W}x{Cin}->3]")
        return y
    if plain and act == ACT_NONE and c1_eligible(Cin, cout, stride):
        # -> one channel (the U-Net discriminator's logit layer): its own kernels, forward and both gradients
        return conv3x3_c1_fwd(x, w_oihw, bias)
    if callable(wp):
        wp = wp()
    fam = _conv_family(wp)
    _conv_flops(N, OH, OW, Cin, cout, fam)
    br = KERNEL_EVENTS.begin("fwd", N, H, W, Cin, cout, stride)
    L = _lib.lib()
    if isinstance(wp, Bf16Packed) and stride == 2:
        assert not ps_out
        rc = L.pesr_conv3x3_bf16_s2(_p(x), _p(wp.t), _p(bias), _p(skip), _p(mask), _p(y), N, H, W, Cin, cout, alpha, act, slope, _stream())
    elif fam is not _DIRECT:
        assert stride == 1
        _conv3x3_wino(x, wp, bias, skip, mask, y, N, H, W, Cin, cout, alpha, act, slope, "fwd", ps_out=ps_out)
        rc = 0
    else:
        nws = L.pesr_conv3x3_workspace_bytes(N, OH, OW, cout)
        ws = workspace(nws, x.device) if nws else None
        rc = L.pesr_conv3x3_fwd(_p(x), _p(wp), _p(bias), _p(skip), _p(mask), _p(y), N, H, W, Cin, cout, stride,
                                alpha, act, slope, int(ps_out), _p(ws), nws, _stream())
    KERNEL_EVENTS.end(br)
    _lib.check(rc, f"pesr_conv3x3_fwd[{N}x{H}x{W}x{Cin}->{cout},s{stride}]")
    return y


def conv3x3_dgrad(dy: torch.Tensor, wpd: torch.Tensor, in_shape, stride: int = 1, alpha: float = 1.0,
                  mask: Optional[torch.Tensor] = None, skip: Optional[torch.Tensor] = None,
                  ps_in: bool = False) -> torch.Tensor:
    """dx for a conv whose forward input had NHWC shape `in_shape`; dy is the (possibly shuffled) output grad."""
    _chk(dy, "conv3x3_dgrad.dy")
    N, H, W, Cin = in_shape
    cout = dy.shape[3] * (4 if ps_in else 1)
    dx = torch.empty((N, H, W, Cin), dtype=torch.float32, device=dy.device)
    _chk_epilogue("conv3x3_dgrad", dx.shape, skip, mask)
    L = _lib.lib()
    fam = _conv_family(wpd)
    _conv_flops(N, (H - 1) // stride + 1, (W - 1) // stride + 1, Cin, cout, fam)
    br = KERNEL_EVENTS.begin("dgrad", N, H, W, Cin, cout, stride)
    if isinstance(wpd, Bf16Packed) and stride == 2:
        assert not ps_in
        rc = L.pesr_conv3x3_bf16_s2_dgrad(_p(dy), _p(wpd.t), _p(mask), _p(skip), _p(dx), N, H, W, cout, Cin, alpha, _stream())
        KERNEL_EVENTS.end(br)
        _lib.check(rc, f"pesr_conv3x3_bf16_s2_dgrad[{N}x{H}x{W}x{Cin}<-{cout}]")
        return dx
    if fam is not _DIRECT:     # the input gradient is the conv of dy with the flipped, transposed kernel
        assert stride == 1
        _conv3x3_wino(dy, wpd, None, skip, mask, dx, N, H, W, cout, Cin, alpha, ACT_NONE, 0.0, "dgrad", ps_in=ps_in)
        KERNEL_EVENTS.end(br)
        return dx
    nws = L.pesr_conv3x3_workspace_bytes(N, H, W, Cin) if stride == 1 else 0
    ws = workspace(nws, dy.device) if nws else None
    rc = L.pesr_conv3x3_dgrad(_p(dy), _p(wpd), _p(mask), _p(skip), _p(dx), N, H, W, Cin, cout, stride, alpha,
                              int(ps_in), _p(ws), nws, _stream())
    KERNEL_EVENTS.end(br)
    _lib.check(rc, f"pesr_conv3x3_dgrad[{N}x{H}x{W}x{Cin}<-{cout},s{stride}]")
    return dx


USE_RGB_IN_DGRAD = True   # tests switch it off to compare with the implicit-GEMM path


def rgb_in_dgrad_eligible(cin: int, cout: int, stride: int) -> bool:
    """Shapes of pesr_conv3x3_rgb_in_dgrad (input gradient of a 3 -> C conv, stride 1)."""
    return USE_RGB_IN_DGRAD and cin == 3 and stride == 1 and cout % 64 == 0 and cout <= 512


def conv3x3_rgb_in_dgrad(dy: torch.Tensor, w_oihw: torch.Tensor, in_shape) -> torch.Tensor:
    """dx of a 3 -> C conv (stride 1, no fused mask): dy [N,H,W,C], w OIHW [C,3,3,3] -> dx [N,H,W,3] (HBM-bound: reads dy once)."""
    _chk(dy, "conv3x3_rgb_in_dgrad.dy"); _chk(w_oihw, "conv3x3_rgb_in_dgrad.w")
    N, H, W, three = in_shape
    C = dy.shape[3]
    assert three == 3 and dy.shape == (N, H, W, C) and w_oihw.shape == (C, 3, 3, 3)
    dx = torch.empty((N, H, W, 3), dtype=torch.float32, device=dy.device)
    _conv_flops(N, H, W, C, 3, _RGB_MFMA)
    br = OP_EVENTS.begin(f"conv_rgb_in_dgrad {C}->3")
    rc = _lib.lib().pesr_conv3x3_rgb_in_dgrad(_p(dy), _p(w_oihw), _p(dx), N, H, W, C, _stream())
    OP_EVENTS.end(br)
    _lib.check(rc, f"pesr_conv3x3_rgb_in_dgrad[{N}x{H}x{W}x3<-{C}]")
    return dx


def conv3x3_rgb_dgrad(dy: torch.Tensor, w_oihw: torch.Tensor, in_shape) -> torch.Tensor:
    """dx of a C -> 3 conv (stride 1, no fused mask): dy [N,H,W,3], w OIHW [3,C,3,3] -> dx [N,H,W,C]."""
    _chk(dy, "conv3x3_rgb_dgrad.dy"); _chk(w_oihw, "conv3x3_rgb_dgrad.w")
    N, H, W, C = in_shape
    assert dy.shape == (N, H, W, 3) and w_oihw.shape == (3, C, 3, 3)
    dx = torch.empty((N, H, W, C), dtype=torch.float32, device=dy.device)
    _conv_flops(N, H, W, C, 3, _RGB_VALU)
    rc = _lib.lib().pesr_conv3x3_rgb_dgrad(_p(dy), _p(w_oihw), _p(dx), N, H, W, C, _stream())
    _lib.check(rc, f"pesr_conv3x3_rgb_dgrad[{N}x{H}x{W}x{C}<-3]")
    return dx


def _out(t, shape, device):
    """Use the caller's output tensor (a view into a flat gradient buffer) when given, else allocate."""
    if t is not None:
        assert tuple(t.shape) == tuple(shape) and t.is_contiguous() and t.dtype == torch.float32
        return t
    return torch.empty(shape, dtype=torch.float32, device=device)


def wgrad_bf16_eligible(N: int, H: int, W: int, Cin: int, Cout: int, stride: int = 1, ps_in: bool = False) -> bool:
    """PRECISION is "bf16" and the bf16 weight-gradient kernel covers the shape (and has at least ~one round of workgroups)."""
    if PRECISION != "bf16" or stride != 1 or W % 48 or Cin % 64 or Cout % 128 or (ps_in and Cout % 512):
        return False
    if _lib.lib().pesr_conv3x3_wgrad_bf16_workspace_bytes(N, H, W, Cin, Cout) == 0:
        return False
    return N * ((H + 1) // 2) * (W // 48) >= (96 if BF16_MIN_WGS >= 64 else 1)


def conv3x3_wgrad_bf16(x: torch.Tensor, dy: torch.Tensor, alpha: float = 1.0, want_bias: bool = True, ps_in: bool = False,
                       dw_out=None, db_out=None, accumulate: bool = False):
    """(dw, db) on the bf16 MFMA: operands rounded to bf16, fp32 sums; db from the un-rounded dy."""
    assert not accumulate or (dw_out is not None and (db_out is not None or not want_bias))
    _chk(x, "conv3x3_wgrad_bf16.x"); _chk(dy, "conv3x3_wgrad_bf16.dy")
    N, H, W, Cin = x.shape
    cout = dy.shape[3] * (4 if ps_in else 1)
    L = _lib.lib()
    nbytes = L.pesr_conv3x3_wgrad_bf16_workspace_bytes(N, H, W, Cin, cout)
    if nbytes == 0:
        raise _lib.PesrHipError(f"pesr_conv3x3_wgrad_bf16: unsupported shape {N}x{H}x{W} Cin={Cin} Cout={cout}")
    ws = workspace(nbytes, x.device)
    dw = _out(dw_out, (cout, Cin, 3, 3), x.device)
    db = _out(db_out, (cout,), x.device) if want_bias else None
    _conv_flops(N, H, W, Cin, cout, _BF16)
    br = KERNEL_EVENTS.begin("wgrad", N, H, W, Cin, cout, 1)
    rc = L.pesr_conv3x3_wgrad_bf16(_p(x), _p(dy), _p(dw), _p(db), N, H, W, Cin, cout, alpha, int(ps_in), int(accumulate), _p(ws),
                                   ws.numel(), _stream())
    KERNEL_EVENTS.end(br)
    _lib.check(rc, f"pesr_conv3x3_wgrad_bf16[{N}x{H}x{W}x{Cin}->{cout}]")
    return dw, db


def conv3x3_wgrad(x: torch.Tensor, dy: torch.Tensor, stride: int = 1, alpha: float = 1.0, want_bias: bool = True,
                  ps_in: bool = False, dw_out=None, db_out=None, algo=None, accumulate: bool = False):
    """(dw [O, I, 3, 3], db [O] | None).  algo: None = by the PESR_* switches (default: auto = F(4,3) where it applies, else
    F(2,3), else direct), or one of WGRAD_AUTO / WGRAD_DIRECT / WGRAD_WINO23.  accumulate: add to dw_out / db_out (which then
    must be given) instead of overwriting them."""
    assert not accumulate or (dw_out is not None and (db_out is not None or not want_bias))
    _chk(x, "conv3x3_wgrad.x")
    _chk(dy, "conv3x3_wgrad.dy")
    N, H, W, Cin = x.shape
    cout = dy.shape[3] * (4 if ps_in else 1)
    if algo is None and wgrad_bf16_eligible(N, H, W, Cin, cout, stride, ps_in):
        return conv3x3_wgrad_bf16(x, dy, alpha, want_bias, ps_in, dw_out, db_out, accumulate)
    L = _lib.lib()
    if algo is None:
        algo = _wgrad_algo()
    nbytes = L.pesr_conv3x3_wgrad_workspace_bytes(N, H, W, Cin, cout, stride, algo)
    if nbytes == 0:
        raise _lib.PesrHipError(f"pesr_conv3x3_wgrad: unsupported shape Cin={Cin} Cout={cout} stride={stride}")
    ws = workspace(nbytes, x.device)
    dw = _out(dw_out, (cout, Cin, 3, 3), x.device)
    db = _out(db_out, (cout,), x.device) if want_bias else None
    _conv_flops(N, (H - 1) // stride + 1, (W - 1) // stride + 1, Cin, cout,
                lambda: _wgrad_kernel(N, H, W, Cin, cout, stride, ps_in, algo, accumulate)[1:])
    br = KERNEL_EVENTS.begin("wgrad", N, H, W, Cin, cout, stride)
    rc = L.pesr_conv3x3_wgrad(_p(x), _p(dy), _p(dw), _p(db), N, H, W, Cin, cout, stride, alpha, int(ps_in), algo, int(accumulate),
                              _p(ws), ws.numel(), _stream())
    KERNEL_EVENTS.end(br)
    _lib.check(rc, f"pesr_conv3x3_wgrad[{N}x{H}x{W}x{Cin}->{cout},s{stride}]")
    return dw, db


def conv3x3_wgrad_rgb(a: torch.Tensor, b3: torch.Tensor, mode: int, alpha: float = 1.0, want_bias: bool = True,
                      dw_out=None, db_out=None, accumulate: bool = False):
    """Weight grad of a conv with a 3-channel side. mode 0: a=dy [N,H,W,C], b3=x -> dw [C,3,3,3]; mode 1: a=x, b3=dy -> dw [3,C,3,3]."""
    _chk(a, "conv3x3_wgrad_rgb.a")
    _chk(b3, "conv3x3_wgrad_rgb.b3")
    N, H, W, C = a.shape
    assert b3.shape == (N, H, W, 3)
    L = _lib.lib()
    nbytes = L.pesr_conv3x3_wgrad_rgb_workspace_bytes(N, H, W, C)
    if nbytes == 0:
        raise _lib.PesrHipError(f"pesr_conv3x3_wgrad_rgb: unsupported channel count {C}")
    ws = workspace(nbytes, a.device)
    dw = _out(dw_out, (C, 3, 3, 3) if mode == 0 else (3, C, 3, 3), a.device)
    db = _out(db_out, (C if mode == 0 else 3,), a.device) if want_bias else None
    _conv_flops(N, H, W, C, 3, _RGB_MFMA if C % 256 == 0 else _RGB_VALU)
    assert not accumulate or (dw_out is not None and not want_bias)
    rc = L.pesr_conv3x3_wgrad_rgb(_p(a), _p(b3), _p(dw), _p(db), N, H, W, C, mode, alpha, int(accumulate), _p(ws), ws.numel(), _stream())
    _lib.check(rc, "pesr_conv3x3_wgrad_rgb")
    return dw, db


# ------------------------------------------------------------------------------------------------
# backward of the upsampler's tail (conv C -> 4C, PixelShuffle(2), conv C -> 3) as one virtual C -> 64 conv: csrc/upsample_tail.hip
# ------------------------------------------------------------------------------------------------
# PESR_UPSAMPLE_TAIL=0: the two convs keep their own autograd nodes everywhere; =1: the collapsed backward wherever it applies; unset
# ("auto"): where it applies AND gains (TAIL_MIN_WORK).  Tests set the attribute.
UPSAMPLE_TAIL = os.environ.get("PESR_UPSAMPLE_TAIL", "auto")
TAIL_CHANNELS = 64      # channels of the virtual conv's output: 3 colours x a 4 x 4 window = 48, padded to what the Winograd kernels take
# What the collapsed backward saves grows with pixels x C^2 (15/16 of the pair's backward flops); composing the virtual weight and chaining
# its gradient back cost the same whatever the image, and it makes eight launches where the two nodes make six.  Measured forward +
# backward of the pair (docs/experiments/upsample_tail.md, "Where it gains"): never slower, but below N H W C^2 = 2^24 both paths are
# launch-bound and the difference (<= 10 us of ~190) is the spread of one path's own repeated runs; at 2^24 it is 8 %, at the training shape 56 %.  "auto"
# takes the path from there up; toy networks and single small patches keep the two nodes and the launch sequence they always had.
TAIL_MIN_WORK = 1 << 24


def upsample_tail_eligible(x: torch.Tensor, c: int) -> bool:
    """The collapsed backward applies - fp32 mode (the bf16 rows keep their own kernels), a GPU tensor [N, H, W, C], C % 16 == 0 - and,
    unless PESR_UPSAMPLE_TAIL=1 asks for it wherever it applies, the problem is large enough for it to gain anything."""
    if UPSAMPLE_TAIL == "0" or PRECISION != "fp32" or not x.is_cuda or c < 16 or c % 16:
        return False
    return UPSAMPLE_TAIL == "1" or x.shape[0] * x.shape[1] * x.shape[2] * c * c >= TAIL_MIN_WORK


def upsample_tail_gather(g: torch.Tensor) -> torch.Tensor:
    """g = dL/d(output) [N, 2H, 2W, 3] -> the window image [N, H, W, 64]: channel (k*4+p)*4+q = g[n, 2y-1+p, 2x-1+q, k], zero outside
    the image and in channels 48..63."""
    _chk(g, "upsample_tail_gather.g")
    N, H2, W2, three = g.shape
    assert three == 3 and H2 % 2 == 0 and W2 % 2 == 0, tuple(g.shape)
    gw = torch.empty((N, H2 // 2, W2 // 2, TAIL_CHANNELS), dtype=torch.float32, device=g.device)
    _lib.check(_lib.lib().pesr_upsample_tail_gather(_p(g), _p(gw), N, H2 // 2, W2 // 2, _stream()), f"pesr_upsample_tail_gather[{N}x{H2}x{W2}]")
    return gw


def upsample_tail_compose(w2: torch.Tensor, w4: torch.Tensor) -> torch.Tensor:
    """(W2 [4C, C, 3, 3], W4 [3, C, 3, 3]) -> the virtual conv's weight [64, C, 3, 3] (OIHW; rows 48..63 zero)."""
    _chk(w2, "upsample_tail_compose.w2"); _chk(w4, "upsample_tail_compose.w4")
    C = w2.shape[1]
    assert tuple(w2.shape) == (4 * C, C, 3, 3) and tuple(w4.shape) == (3, C, 3, 3), (tuple(w2.shape), tuple(w4.shape))
    weff = torch.empty((TAIL_CHANNELS, C, 3, 3), dtype=torch.float32, device=w2.device)
    _lib.check(_lib.lib().pesr_upsample_tail_compose(_p(w2), _p(w4), _p(weff), C, _stream()), f"pesr_upsample_tail_compose[C={C}]")
    return weff


def upsample_tail_chain(w2: torch.Tensor, b2: Optional[torch.Tensor], w4: torch.Tensor, S: torch.Tensor, T: torch.Tensor,
                        want=(True, True, True, True), outs=(None, None, None, None), accumulate: bool = False):
    """The virtual conv's weight gradient S [64, C, 3, 3] and bias gradient T [64] -> (dW2, db2, dW4, db4), None where `want` is
    False.  outs: the tensors to write (flat-gradient views), None: fresh ones.  accumulate: add to `outs` (which then must be given)."""
    for t, n in ((w2, "w2"), (w4, "w4"), (S, "S"), (T, "T")) + (((b2, "b2"),) if b2 is not None else ()):
        _chk(t, f"upsample_tail_chain.{n}")
    C = w2.shape[1]
    assert tuple(w2.shape) == (4 * C, C, 3, 3) and tuple(w4.shape) == (3, C, 3, 3) and tuple(S.shape) == (TAIL_CHANNELS, C, 3, 3)
    assert tuple(T.shape) == (TAIL_CHANNELS,) and (b2 is None or tuple(b2.shape) == (4 * C,))
    assert not accumulate or all(o is not None for o, wnt in zip(outs, want) if wnt)
    shapes = ((4 * C, C, 3, 3), (4 * C,), (3, C, 3, 3), (3,))
    res = [_out(o, shp, w2.device) if wnt else None for o, shp, wnt in zip(outs, shapes, want)]
    if any(want):
        rc = _lib.lib().pesr_upsample_tail_chain(_p(w2), _p(b2), _p(w4), _p(S), _p(T), *(_p(r) for r in res), C, int(accumulate), _stream())
        _lib.check(rc, f"pesr_upsample_tail_chain[C={C}]")
    return tuple(res)


# ------------------------------------------------------------------------------------------------
# MeanShift / PixelShuffle / masks / pooling
# ------------------------------------------------------------------------------------------------
def meanshift_fwd(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, x_nchw: bool = False, y_nchw: bool = False):
    """x: [N,H,W,3] (or [N,3,H,W] contiguous when x_nchw) -> y in NHWC (or NCHW when y_nchw)."""
    _chk(x, "meanshift_fwd.x")
    if x_nchw:
        N, _, H, W = x.shape
    else:
        N, H, W, _ = x.shape
    y = torch.empty((N, 3, H, W) if y_nchw else (N, H, W, 3), dtype=torch.float32, device=x.device)
    br = OP_EVENTS.begin(f"meanshift {H}x{W}")
    rc = _lib.lib().pesr_meanshift_fwd(_p(x), _p(w), _p(b), _p(y), N, H, W, int(x_nchw), int(y_nchw), _stream())
    OP_EVENTS.end(br)
    _lib.check(rc, "pesr_meanshift_fwd")
    return y


def meanshift_bwd(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor, x_nchw: bool = False, need_dx: bool = True,
                  dw_out=None, db_out=None):
    _chk(dy, "meanshift_bwd.dy")
    N, H, W, _ = dy.shape
    dx = torch.empty_like(dy) if need_dx else None
    dw = _out(dw_out, (3, 3, 1, 1), dy.device)
    db = _out(db_out, (3,), dy.device)
    ws = workspace(1024 * 12 * 4 + 128, dy.device)
    rc = _lib.lib().pesr_meanshift_bwd(_p(dy), _p(x), _p(w), _p(dx), _p(dw), _p(db), N, H, W, int(x_nchw), _p(ws),
                                       ws.numel(), _stream())
    _lib.check(rc, "pesr_meanshift_bwd")
    return dx, dw, db


def pixel_shuffle_fwd(x: torch.Tensor) -> torch.Tensor:
    _chk(x, "pixel_shuffle_fwd.x")
    N, H, W, C4 = x.shape
    y = torch.empty((N, 2 * H, 2 * W, C4 // 4), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().pesr_pixel_shuffle_fwd(_p(x), _p(y), N, H, W, C4 // 4, _stream()), "pesr_pixel_shuffle_fwd")
    return y


def pixel_shuffle_bwd(dy: torch.Tensor) -> torch.Tensor:
    _chk(dy, "pixel_shuffle_bwd.dy")
    N, H2, W2, C = dy.shape
    dx = torch.empty((N, H2 // 2, W2 // 2, 4 * C), dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib().pesr_pixel_shuffle_bwd(_p(dy), _p(dx), N, H2 // 2, W2 // 2, C, _stream()), "pesr_pixel_shuffle_bwd")
    return dx


def pixel_shuffle_r_fwd(x: torch.Tensor, r: int) -> torch.Tensor:
    """nn.PixelShuffle(r), r in {2, 3}, NHWC: x [N,H,W,r*r*C] -> y [N,r*H,r*W,C] (torch's channel order)."""
    _chk(x, "pixel_shuffle_r_fwd.x")
    N, H, W, Crr = x.shape
    if r not in (2, 3) or Crr % (r * r):
        raise _lib.PesrHipError(f"pixel_shuffle_r_fwd: r = {r} with {Crr} channels (r must be 2 or 3, channels a multiple of r*r)")
    C = Crr // (r * r)
    y = torch.empty((N, r * H, r * W, C), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().pesr_pixel_shuffle_r_fwd(_p(x), _p(y), N, H, W, C, r, _stream()), f"pesr_pixel_shuffle_r_fwd[r={r}]")
    return y


def pixel_shuffle_r_bwd(dy: torch.Tensor, r: int) -> torch.Tensor:
    """Its backward (nn.PixelUnshuffle(r)): dy [N,r*H,r*W,C] -> dx [N,H,W,r*r*C]."""
    _chk(dy, "pixel_shuffle_r_bwd.dy")
    N, HR, WR, C = dy.shape
    if r not in (2, 3) or HR % r or WR % r:
        raise _lib.PesrHipError(f"pixel_shuffle_r_bwd: r = {r} with a {HR}x{WR} gradient (r must be 2 or 3 and divide both sizes)")
    dx = torch.empty((N, HR // r, WR // r, r * r * C), dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib().pesr_pixel_shuffle_r_bwd(_p(dy), _p(dx), N, HR // r, WR // r, C, r, _stream()), f"pesr_pixel_shuffle_r_bwd[r={r}]")
    return dx


def relu_mask(g: torch.Tensor, ref: Optional[torch.Tensor] = None, add: Optional[torch.Tensor] = None,
              alpha: float = 1.0, slope: float = 0.0) -> torch.Tensor:
    _chk(g, "relu_mask.g")
    out = torch.empty_like(g)
    _lib.check(_lib.lib().pesr_relu_mask(_p(g), _p(ref), _p(add), _p(out), g.numel(), alpha, slope, _stream()), "pesr_relu_mask")
    return out


def maxpool2x2_fwd(x: torch.Tensor) -> torch.Tensor:
    _chk(x, "maxpool2x2_fwd.x")
    N, H, W, C = x.shape
    y = torch.empty((N, H // 2, W // 2, C), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().pesr_maxpool2x2_fwd(_p(x), _p(y), N, H, W, C, _stream()), "pesr_maxpool2x2_fwd")
    return y


def maxpool2x2_bwd(x: torch.Tensor, dy: torch.Tensor, relu_in: bool) -> torch.Tensor:
    _chk(dy, "maxpool2x2_bwd.dy")
    N, H, W, C = x.shape
    dx = torch.empty_like(x)
    _lib.check(_lib.lib().pesr_maxpool2x2_bwd(_p(x), _p(dy), _p(dx), N, H, W, C, int(relu_in), _stream()), "pesr_maxpool2x2_bwd")
    return dx


# ------------------------------------------------------------------------------------------------
# BatchNorm(train) + LeakyReLU
# ------------------------------------------------------------------------------------------------
def _bn_y(x, y_nchw):
    """The output of a BatchNorm + activation over x [N,H,W,C]: NHWC, or NCHW (the flatten in front of the classifier)."""
    N, H, W, C = x.shape
    return torch.empty((N, C, H, W) if y_nchw else (N, H, W, C), dtype=torch.float32, device=x.device)


def bn_lrelu_fwd(x, gamma, beta, running_mean, running_var, num_batches, eps=1e-5, momentum=0.1, slope=0.2,
                 y_nchw=False):
    _chk(x, "bn_lrelu_fwd.x")
    N, H, W, C = x.shape
    L = _lib.lib()
    ws = workspace(L.pesr_bn_workspace_bytes(N * H * W, C), x.device)
    y = _bn_y(x, y_nchw)
    stats = torch.empty((2, C), dtype=torch.float32, device=x.device)
    rc = L.pesr_bn_lrelu_fwd(_p(x), _p(gamma), _p(beta), _p(y), _p(stats), _p(running_mean), _p(running_var),
                             _p(num_batches), N, H, W, C, eps, momentum, slope, int(y_nchw), _p(ws), ws.numel(), _stream())
    _lib.check(rc, "pesr_bn_lrelu_fwd")
    return y, stats


def conv_rgb_bn_eligible(cin: int, cout: int, stride: int) -> bool:
    """Shapes of pesr_conv3x3_rgb_bn_lrelu_fwd (3 -> C conv whose kernel also leaves the BatchNorm partial sums)."""
    return rgb_in_eligible(cin, cout, stride)


def conv_rgb_bn_lrelu_fwd(x, w_oihw, gamma, beta, running_mean, running_var, num_batches, eps=1e-5, momentum=0.1, slope=0.2,
                          y_nchw=False):
    """(z, y, stats): z = conv3x3(x [N,H,W,3], w) without bias, y = act(bn_train(z)); the statistics come out of the conv kernel's
    epilogue (no pass over z for them)."""
    _chk(x, "conv_rgb_bn_lrelu_fwd.x"); _chk(w_oihw, "conv_rgb_bn_lrelu_fwd.w")
    N, H, W, Cin = x.shape
    C = w_oihw.shape[0]
    assert tuple(w_oihw.shape) == (C, 3, 3, 3) and conv_rgb_bn_eligible(Cin, C, 1)
    L = _lib.lib()
    ws = workspace(L.pesr_conv3x3_rgb_bn_workspace_bytes(N, H, W, C), x.device)
    z = torch.empty((N, H, W, C), dtype=torch.float32, device=x.device)
    y = _bn_y(z, y_nchw)
    stats = torch.empty((2, C), dtype=torch.float32, device=x.device)
    _conv_flops(N, H, W, Cin, C, _RGB_VALU)
    rc = L.pesr_conv3x3_rgb_bn_lrelu_fwd(_p(x), _p(w_oihw), _p(z), _p(gamma), _p(beta), _p(y), _p(stats), _p(running_mean), _p(running_var),
                                         _p(num_batches), N, H, W, C, eps, momentum, slope, int(y_nchw), _p(ws), ws.numel(), _stream())
    _lib.check(rc, f"pesr_conv3x3_rgb_bn_lrelu_fwd[{N}x{H}x{W}x3->{C}]")
    return z, y, stats


# ---- convs whose epilogue leaves the BatchNorm sums (round 6; include/pesr_hip.h PesrBnFuse) -------------------------------------------
class _BnFuse(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("rows", ctypes.c_int), ("part", ctypes.c_void_p),
                ("z", ctypes.c_void_p), ("mean_invstd", ctypes.c_void_p), ("gamma", ctypes.c_void_p),
                ("beta", ctypes.c_void_p), ("slope", ctypes.c_float)]


BN_FWD_STATS, BN_BWD_MASK_SUMS = 1, 2
USE_BN_FUSE = os.environ.get("PESR_BN_FUSE", "1") != "0"     # PESR_BN_FUSE=0: the un-fused BatchNorm passes everywhere (A/B switch)
_BN_ROWS = {}


def conv_bn_rows(which: int, N: int, H: int, W: int, Cin: int, Cout: int, stride: int = 1) -> int:
    """Rows of BatchNorm sums the fused call `which` (0 = conv3x3_fwd_bn on direct packing, 1 = conv3x3_dgrad_bn on direct dgrad packing,
    2 = the F(4,3) kernel) leaves for this problem; 0: not covered (split-K layers, odd channel counts) - use the un-fused calls."""
    if not USE_BN_FUSE:
        return 0
    return _memo("pesr_conv3x3_bn_rows", which, N, H, W, Cin, Cout, stride, cache=_BN_ROWS)


def _fuse_struct(mode, part, z=None, stats=None, gamma=None, beta=None, slope=0.0):
    f = _BnFuse()
    f.mode, f.rows, f.part = mode, part.shape[0], part.data_ptr()
    f.z, f.mean_invstd, f.gamma, f.beta, f.slope = _p(z), _p(stats), _p(gamma), _p(beta), float(slope)
    return f


def _conv3x3_bn(kind, src, wp, bias, N, H, W, Cin, cout, stride, mode, **bn):
    """A conv [N,H,W,Cin] -> cout whose kernel leaves BatchNorm sums: kind "fwd" runs it on src = x, kind "dgrad" its input gradient on
    src = dy -> (out, part [rows, 2, channels of out]) or None when the fused form does not cover this problem / packing."""
    fwd = kind == "fwd"
    four = isinstance(wp, Wino4Packed)
    if not four and not torch.is_tensor(wp):
        return None
    ci, co = (Cin, cout) if fwd else (cout, Cin)        # channels of src and of out; the F(4,3) kernel (stride 1) runs ci -> co either way
    rows = conv_bn_rows(2, N, H, W, ci, co, 1) if four else conv_bn_rows(0 if fwd else 1, N, H, W, Cin, cout, stride)
    if rows == 0:
        return None
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    oshape = (N, OH, OW, co) if fwd else (N, H, W, co)
    L = _lib.lib()
    out = torch.empty(oshape, dtype=torch.float32, device=src.device)
    part = torch.empty((rows, 2, co), dtype=torch.float32, device=src.device)
    f = _fuse_struct(mode, part, **bn)
    nws = L.pesr_conv3x3_workspace_bytes(*oshape) if fwd or stride == 1 else 0
    ws = workspace(nws, src.device) if nws else None
    _conv_flops(N, OH, OW, Cin, cout, _conv_family(wp))
    br = KERNEL_EVENTS.begin(kind, N, H, W, Cin, cout, stride)
    if four:
        rc = L.pesr_conv3x3_wino4_bn(_p(src), _p(wp.t), _p(bias), _p(out), N, H, W, ci, co, _p(ws), nws, ctypes.byref(f), _stream())
    elif fwd:
        rc = L.pesr_conv3x3_fwd_bn(_p(src), _p(wp), _p(bias), _p(out), N, H, W, Cin, cout, stride, _p(ws), nws, ctypes.byref(f), _stream())
    else:
        rc = L.pesr_conv3x3_dgrad_bn(_p(src), _p(wp), _p(out), N, H, W, Cin, cout, stride, _p(ws), nws, ctypes.byref(f), _stream())
    KERNEL_EVENTS.end(br)
    _lib.check(rc, f"pesr_conv3x3_{'wino4' if four else kind}_bn[{N}x{H}x{W}x{Cin}{'->' if fwd else '<-'}{cout},s{stride}]")
    return out, part


def conv3x3_fwd_bn_stats(x: torch.Tensor, wp, bias: Optional[torch.Tensor], cout: int, stride: int = 1):
    """z = conv(x) (+ bias) with the per-pixel-tile sums of z and z^2 left by the kernel's epilogue -> (z, part [rows, 2, cout]) or None when
    the fused form does not cover this problem / packing (the caller then runs conv3x3_fwd + bn_lrelu_fwd)."""
    _chk(x, "conv3x3_fwd_bn_stats.x")
    return _conv3x3_bn("fwd", x, wp, bias, *x.shape, cout, stride, BN_FWD_STATS)


def bn_finalize_apply(z, part, gamma, beta, running_mean, running_var, num_batches, eps=1e-5, momentum=0.1, slope=0.2, y_nchw=False):
    """The BatchNorm of z from the sums a conv kernel left (conv3x3_fwd_bn_stats): finalize + apply -> (y, stats [2, C])."""
    N, H, W, C = z.shape
    L = _lib.lib()
    stats = torch.empty((2, C), dtype=torch.float32, device=z.device)
    _lib.check(L.pesr_bn_finalize(_p(part), part.shape[0], C, N * H * W, eps, momentum, _p(stats), _p(running_mean), _p(running_var),
                                  _p(num_batches), _stream()), "pesr_bn_finalize")
    y = _bn_y(z, y_nchw)
    _lib.check(L.pesr_bn_lrelu_eval_fwd(_p(z), _p(gamma), _p(beta), _p(stats), _p(y), N, H, W, C, slope, int(y_nchw), _stream()), "pesr_bn_lrelu_eval_fwd")
    return y, stats


def conv3x3_dgrad_bn_sums(dy: torch.Tensor, wpd, in_shape, stride, z, stats, gamma, beta, slope):
    """The input gradient dx of a conv whose INPUT was y = lrelu(bn(z)): the kernel stores g' = dx * lrelu'(bn(z)) and leaves the sums of g'
    and g' * xhat per pixel tile -> (g' [in_shape], part [rows, 2, C]) or None when the fused form does not cover the problem / packing."""
    _chk(dy, "conv3x3_dgrad_bn_sums.dy")
    assert tuple(z.shape) == tuple(in_shape) and z.is_contiguous()
    return _conv3x3_bn("dgrad", dy, wpd, None, *in_shape, dy.shape[3], stride, BN_BWD_MASK_SUMS, z=z, stats=stats, gamma=gamma, beta=beta,
                       slope=slope)


def _bn_param_grads(need_param_grads, dgamma_out, dbeta_out, C, device):
    """(dgamma, dbeta) [C]: the caller's tensors where given, fresh ones else; (None, None) when not wanted."""
    if not need_param_grads:
        return None, None
    return _out(dgamma_out, (C,), device), _out(dbeta_out, (C,), device)


def bn_lrelu_backward(x, dy, gamma, beta, stats, slope=0.2, dy_nchw=False, need_param_grads=True, dgamma_out=None, dbeta_out=None,
                      accumulate=False, training=True, part=None):
    """Backward of y = lrelu(bn(x)) -> (dx, dgamma, dbeta).  training: batch statistics (bn_lrelu_bwd), else the running ones
    (bn_lrelu_eval_bwd).  part: dy already is the masked gradient and part holds the sums its conv kernel left (bn_lrelu_bwd_fused).
    accumulate: add to dgamma_out / dbeta_out (which then must be given) instead of overwriting them."""
    fused = part is not None
    fn = "bn_lrelu_bwd_fused" if fused else "bn_lrelu_bwd" if training else "bn_lrelu_eval_bwd"
    _chk(dy, fn + (".g" if fused else ".dy"))
    assert not accumulate or (dgamma_out is not None and dbeta_out is not None and (fused or training))
    N, H, W, C = x.shape
    L = _lib.lib()
    ws = workspace(2 * C * 4 + 256 if fused else L.pesr_bn_workspace_bytes(N * H * W, C), x.device)
    dx = torch.empty_like(x)
    dgamma, dbeta = _bn_param_grads(need_param_grads, dgamma_out, dbeta_out, C, x.device)
    sums = (_p(part), part.shape[0]) if fused else ()
    how = (int(accumulate),) if fused else (slope, int(dy_nchw), int(accumulate)) if training else (slope, int(dy_nchw))
    rc = getattr(L, "pesr_" + fn)(_p(x), _p(dy), *sums, _p(gamma), _p(beta), _p(stats), _p(dx), _p(dgamma), _p(dbeta), N, H, W, C, *how,
                                  _p(ws), ws.numel(), _stream())
    _lib.check(rc, "pesr_" + fn)
    return dx, dgamma, dbeta


def bn_lrelu_bwd_fused(z, g_masked, part, gamma, beta, stats, need_param_grads=True, dgamma_out=None, dbeta_out=None, accumulate=False):
    """BatchNorm backward from the sums the producing conv kernel left (conv3x3_dgrad_bn_sums): -> (dz, dgamma, dbeta)."""
    return bn_lrelu_backward(z, g_masked, gamma, beta, stats, 0.0, False, need_param_grads, dgamma_out, dbeta_out, accumulate, True, part)


def bn_lrelu_bwd(x, dy, gamma, beta, stats, slope=0.2, dy_nchw=False, need_param_grads=True, dgamma_out=None, dbeta_out=None,
                 accumulate=False):
    return bn_lrelu_backward(x, dy, gamma, beta, stats, slope, dy_nchw, need_param_grads, dgamma_out, dbeta_out, accumulate)


def bn_bwd_bwd(z, du, g, gamma, stats, need_du=True, need_z=True, need_gamma=True):
    """Backward of the training-mode BatchNorm backward (pesr_bn_bwd_bwd): (dL/d(du), dL/dz, dL/dgamma) for g = dL/d(dz)."""
    for t, n in ((z, "z"), (du, "du"), (g, "g")):
        _chk(t, "bn_bwd_bwd." + n)
    N, H, W, C = z.shape
    L = _lib.lib()
    ws = workspace(L.pesr_bn_bwd_bwd_workspace_bytes(N * H * W, C), z.device)
    l_du = torch.empty_like(z) if need_du else None
    l_z = torch.empty_like(z) if need_z else None
    l_ga = torch.empty((C,), dtype=torch.float32, device=z.device) if need_gamma else None
    rc = L.pesr_bn_bwd_bwd(_p(z), _p(du), _p(g), _p(gamma), _p(stats), _p(l_du), _p(l_z), _p(l_ga), N, H, W, C, _p(ws), ws.numel(), _stream())
    _lib.check(rc, "pesr_bn_bwd_bwd")
    return l_du, l_z, l_ga


def bn_eval_stats(running_mean, running_var, eps=1e-5):
    """[2, C] {mean, invstd} of an eval-mode BatchNorm2d from its running statistics (C-sized torch glue)."""
    return torch.stack([running_mean.float(), torch.rsqrt(running_var.float() + eps)]).contiguous()


def bn_lrelu_eval_fwd(x, gamma, beta, stats, slope=0.2, y_nchw=False):
    _chk(x, "bn_lrelu_eval_fwd.x")
    N, H, W, C = x.shape
    y = _bn_y(x, y_nchw)
    rc = _lib.lib().pesr_bn_lrelu_eval_fwd(_p(x), _p(gamma), _p(beta), _p(stats), _p(y), N, H, W, C, slope, int(y_nchw), _stream())
    _lib.check(rc, "pesr_bn_lrelu_eval_fwd")
    return y


def bn_lrelu_eval_bwd(x, dy, gamma, beta, stats, slope=0.2, dy_nchw=False, need_param_grads=True, dgamma_out=None, dbeta_out=None):
    return bn_lrelu_backward(x, dy, gamma, beta, stats, slope, dy_nchw, need_param_grads, dgamma_out, dbeta_out, training=False)


# ------------------------------------------------------------------------------------------------
# Linear
# ------------------------------------------------------------------------------------------------
LIN_MAXM = 32     # rows per kernel call (pesr_hip.h); larger batches are walked in chunks


def linear_fwd(x, w, b, act=ACT_NONE, slope=0.0):
    _chk(x, "linear_fwd.x")
    M, K = x.shape
    Nf = w.shape[0]
    L = _lib.lib()
    y = torch.empty((M, Nf), dtype=torch.float32, device=x.device)
    FLOPS.add(2.0 * M * Nf * K, 1.0, "linear (HBM-bound, MFMA)")
    for m0 in range(0, M, LIN_MAXM):
        m = min(LIN_MAXM, M - m0)
        ws = workspace(L.pesr_linear_workspace_bytes(m, Nf, K), x.device)
        _lib.check(L.pesr_linear_fwd(_p(x[m0:m0 + m]), _p(w), _p(b), _p(y[m0:m0 + m]), m, Nf, K, act, slope, _p(ws), ws.numel(), _stream()),
                   "pesr_linear_fwd")
    return y


def linear_dgrad(dy, w, out=None):
    """out: the [M, K] tensor (or leading rows of a larger one) the gradient is written into."""
    _chk(dy, "linear_dgrad.dy")
    M, Nf = dy.shape
    K = w.shape[1]
    L = _lib.lib()
    if out is not None:
        _chk(out, "linear_dgrad.out")
        assert tuple(out.shape) == (M, K)
    dx = out if out is not None else torch.empty((M, K), dtype=torch.float32, device=dy.device)
    FLOPS.add(2.0 * M * Nf * K, 0.0, "linear (HBM-bound, VALU)")
    for m0 in range(0, M, LIN_MAXM):
        m = min(LIN_MAXM, M - m0)
        ws = workspace(L.pesr_linear_workspace_bytes(m, Nf, K), dy.device)
        _lib.check(L.pesr_linear_dgrad(_p(dy[m0:m0 + m]), _p(w), _p(dx[m0:m0 + m]), m, Nf, K, _p(ws), ws.numel(), _stream()), "pesr_linear_dgrad")
    return dx


def linear_wgrad(dy, x, want_bias=True, dw_out=None, db_out=None, accumulate=False):
    """accumulate: add to dw_out / db_out (which then must be given) instead of overwriting them."""
    _chk(dy, "linear_wgrad.dy")
    M, Nf = dy.shape
    K = x.shape[1]
    assert not accumulate or (dw_out is not None and (db_out is not None or not want_bias))
    dw = _out(dw_out, (Nf, K), dy.device)
    db = _out(db_out, (Nf,), dy.device) if want_bias else None
    FLOPS.add(2.0 * M * Nf * K, 0.0, "linear (HBM-bound, VALU)")
    for m0 in range(0, M, LIN_MAXM):
        m = min(LIN_MAXM, M - m0)
        _lib.check(_lib.lib().pesr_linear_wgrad(_p(dy[m0:m0 + m]), _p(x[m0:m0 + m]), _p(dw), _p(db), m, Nf, K, int(accumulate or m0 > 0), _stream()),
                   "pesr_linear_wgrad")
    return dw, db


# ------------------------------------------------------------------------------------------------
# losses / optimizer
# ------------------------------------------------------------------------------------------------
def loss_l1_tv(sr, hr, g_l1: float, g_tv: float, need_grad=True):
    """-> (out2 device tensor [l1_mean, tv_sum], grad [N,H,W,3] | None)"""
    _chk(sr, "loss_l1_tv.sr")
    _chk(hr, "loss_l1_tv.hr")
    N, H, W, _ = sr.shape
    out = torch.empty((2,), dtype=torch.float32, device=sr.device)
    grad = torch.empty_like(sr) if need_grad else None
    ws = workspace(16384, sr.device)
    rc = _lib.lib().pesr_loss_l1_tv_fwd_bwd(_p(sr), _p(hr), _p(grad), _p(out), N, H, W, g_l1, g_tv, _p(ws), ws.numel(), _stream())
    _lib.check(rc, "pesr_loss_l1_tv_fwd_bwd")
    return out, grad


def loss_mse(a, b, gscale: float, need_grad=True):
    _chk(a, "loss_mse.a")
    _chk(b, "loss_mse.b")
    out = torch.empty((1,), dtype=torch.float32, device=a.device)
    grad = torch.empty_like(a) if need_grad else None
    ws = workspace(16384, a.device)
    rc = _lib.lib().pesr_mse_fwd_bwd(_p(a), _p(b), _p(grad), _p(out), a.numel(), gscale, _p(ws), ws.numel(), _stream())
    _lib.check(rc, "pesr_mse_fwd_bwd")
    return out, grad


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0):
    for t, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _chk(t, f"adam_step.{n}")
    rc = _lib.lib().pesr_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, step, grad_scale, _stream())
    _lib.check(rc, "pesr_adam_step")


def adam_step_dev(p, g, m, v, state, beta1, beta2, eps, grad_scale=1.0):
    """Adam step whose learning rate and step count live in the 6-float device tensor `state` (include/pesr_hip.h): safe to
    capture in a hipGraph - nothing that changes from step to step is a kernel argument."""
    for t, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v"), (state, "state")):
        _chk(t, f"adam_step_dev.{n}")
    assert state.numel() == 6
    rc = _lib.lib().pesr_adam_step_dev(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(state), beta1, beta2, eps, grad_scale, _stream())
    _lib.check(rc, "pesr_adam_step_dev")


def adam_ema_step(p, g, m, v, ema, ema_decay, lr, beta1, beta2, eps, step, grad_scale=1.0):
    """adam_step plus ema += (p_new - ema) * (1 - ema_decay) in the same launch; p, m, v exactly as adam_step leaves them."""
    for t, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v"), (ema, "ema")):
        _chk(t, f"adam_ema_step.{n}")
    assert ema.numel() == p.numel()
    rc = _lib.lib().pesr_adam_ema_step(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, step, grad_scale, _p(ema),
                                       ema_decay, _stream())
    _lib.check(rc, "pesr_adam_ema_step")


def adam_ema_step_dev(p, g, m, v, ema, ema_decay, state, beta1, beta2, eps, grad_scale=1.0):
    """adam_step_dev plus the moving average of adam_ema_step: capturable, the average is updated inside the replayed launch."""
    for t, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v"), (ema, "ema"), (state, "state")):
        _chk(t, f"adam_ema_step_dev.{n}")
    assert state.numel() == 6 and ema.numel() == p.numel()
    rc = _lib.lib().pesr_adam_ema_step_dev(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(state), beta1, beta2, eps, grad_scale, _p(ema),
                                           ema_decay, _stream())
    _lib.check(rc, "pesr_adam_ema_step_dev")


def _image_layout(t, err: str, min_n: int = 0, max_n: Optional[int] = None):
    """[n, 3, h, w] fp32 device tensor -> (tensor, 0 if NCHW-contiguous / 1 if channels_last).  A tensor in neither layout is copied
    by torch first; anything else, or n outside min_n .. max_n, raises `err`."""
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != 3 \
            or t.shape[0] < min_n or (max_n is not None and t.shape[0] > max_n):
        raise _lib.PesrHipError(err)
    if t.is_contiguous():
        return t, 0
    if t.is_contiguous(memory_format=torch.channels_last):
        return t, 1
    return t.contiguous(), 0


def psnr_y(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Y-channel PSNR of two [1, 3, H, W] image tensors (NCHW-contiguous or channels_last) -> device double [mse, psnr]."""
    (ta, la), (tb, lb) = (_image_layout(t, "psnr_y: expected [1, 3, H, W] float32 GPU tensors", 1, 1) for t in (a, b))
    assert ta.shape == tb.shape
    H, W = ta.shape[2], ta.shape[3]
    out = torch.empty(2, dtype=torch.float64, device=ta.device)
    ws = workspace(4096, ta.device)
    rc = _lib.lib().pesr_psnr_y(ta.data_ptr(), tb.data_ptr(), out.data_ptr(), H, W, la, lb, ws.data_ptr(), ws.numel(), _stream())
    _lib.check(rc, "pesr_psnr_y")
    return out


# g[k] = exp(-(k-5)^2 / 4.5) / sum, k = 0..10: the SSIM window (docs/modes.md section 4g).  ssim.hip carries these doubles as literals;
# utils.compute_SSIM's host path filters with them.
SSIM_WINDOW = (0.00102838008447911, 0.007598758135239185, 0.03600077212843083, 0.10936068950970002, 0.2130055377112537,
               0.26601172486179436, 0.2130055377112537, 0.10936068950970002, 0.03600077212843083, 0.007598758135239185,
               0.00102838008447911)


def _ssim_loss_pair(what: str, a: torch.Tensor, b: torch.Tensor, shave=None):
    """The checks of ssim_y (with its shave) and of the loss's two halves (shave None) -> the tensors, their layouts, N, H, W and the
    size Ho x Wo of the map."""
    (ta, la), (tb, lb) = (_image_layout(t, f"{what}: expected [N, 3, H, W] float32 GPU tensors", 1) for t in (a, b))
    if ta.shape != tb.shape:
        raise ValueError(f"{what}: the two tensors differ in shape: {tuple(ta.shape)} and {tuple(tb.shape)}")
    N, H, W = ta.shape[0], ta.shape[2], ta.shape[3]
    Ho, Wo = H - 2 * (shave or 0) - 10, W - 2 * (shave or 0) - 10
    if (shave or 0) < 0 or Ho < 1 or Wo < 1:
        why = "is smaller than" if shave is None else f"with shave {shave} leaves less than"
        raise ValueError(f"{what}: a {H} x {W} image {why} the 11 x 11 window")
    return ta, la, tb, lb, N, H, W, Ho, Wo


def _ssim_workspace(N: int, Ho: int, Wo: int, device):
    """One double per tile of the map; counted with 16 x 16 tiles, which is no fewer than either kernel's tile gives."""
    return workspace(8 * N * ((Ho + 15) // 16) * ((Wo + 15) // 16), device)


def ssim_y(a: torch.Tensor, b: torch.Tensor, shave: int = 0, return_map: bool = False):
    """Y-channel SSIM of N image pairs [N, 3, H, W] (each NCHW-contiguous or channels_last), a border of `shave` pixels ignored
    -> device double [N], the mean of each pair's map; with return_map also the [N, H-2*shave-10, W-2*shave-10] double map."""
    shave = int(shave)
    ta, la, tb, lb, N, H, W, Ho, Wo = _ssim_loss_pair("ssim_y", a, b, shave)
    out = torch.empty(N, dtype=torch.float64, device=ta.device)
    smap = torch.empty((N, Ho, Wo), dtype=torch.float64, device=ta.device) if return_map else None
    ws = _ssim_workspace(N, Ho, Wo, ta.device)
    rc = _lib.lib().pesr_ssim_y(ta.data_ptr(), tb.data_ptr(), out.data_ptr(), N, H, W, la, lb, shave,
                                smap.data_ptr() if return_map else None, ws.data_ptr(), ws.numel(), _stream())
    _lib.check(rc, "pesr_ssim_y")
    return (out, smap) if return_map else out


def ssim_loss_fwd(a: torch.Tensor, b: torch.Tensor, need_grad: bool = False):
    """SSIM-Y on the unquantised luma (docs/modes.md section 4p) of N image pairs [N, 3, H, W], each NCHW-contiguous or channels_last
    -> (device double [N], the mean of each pair's map; coef).  coef is None unless need_grad: then the double [N, 3, H-10, W-10] of
    each window's derivatives with respect to mean(x), mean(x*x) and mean(x*y), what ssim_loss_bwd reads."""
    ta, la, tb, lb, N, H, W, Ho, Wo = _ssim_loss_pair("ssim_loss_fwd", a, b)
    score = torch.empty(N, dtype=torch.float64, device=ta.device)
    coef = torch.empty((N, 3, Ho, Wo), dtype=torch.float64, device=ta.device) if need_grad else None
    ws = _ssim_workspace(N, Ho, Wo, ta.device)
    rc = _lib.lib().pesr_ssim_loss_fwd(ta.data_ptr(), tb.data_ptr(), score.data_ptr(), N, H, W, la, lb,
                                       coef.data_ptr() if need_grad else None, ws.data_ptr(), ws.numel(), _stream())
    _lib.check(rc, "pesr_ssim_loss_fwd")
    return score, coef


def ssim_loss_bwd(a: torch.Tensor, b: torch.Tensor, coef: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """The gradient of ssim_loss_fwd(a, b)'s score with respect to a (docs/modes.md section 4p).  coef: what the forward returned for the
    same pair; g: device double [N], dL/dscore of each pair -> fp32 [N, 3, H, W] with a's strides.  b gets none."""
    ta, la, tb, lb, N, H, W, Ho, Wo = _ssim_loss_pair("ssim_loss_bwd", a, b)
    if not torch.is_tensor(coef) or not coef.is_cuda or coef.dtype != torch.float64 or tuple(coef.shape) != (N, 3, Ho, Wo) \
            or not coef.is_contiguous():
        raise _lib.PesrHipError(f"ssim_loss_bwd.coef: expected a contiguous float64 GPU tensor [{N}, 3, {Ho}, {Wo}]")
    if not torch.is_tensor(g) or not g.is_cuda or g.dtype != torch.float64 or tuple(g.shape) != (N,) or not g.is_contiguous():
        raise _lib.PesrHipError(f"ssim_loss_bwd.g: expected a contiguous float64 GPU tensor [{N}]")
    ga = torch.empty_like(ta)                  # (preserve_format: ta is dense in one of the two layouts, so these are its strides)
    rc = _lib.lib().pesr_ssim_loss_bwd(ta.data_ptr(), tb.data_ptr(), coef.data_ptr(), g.data_ptr(), ga.data_ptr(), N, H, W, la, lb,
                                       _stream())
    _lib.check(rc, "pesr_ssim_loss_bwd")
    return ga


LPIPS_CHANNELS = (64, 128, 256, 512)


def lpips_layer(feat: torch.Tensor, w: torch.Tensor, return_map: bool = False):
    """The LPIPS head of one tapped layer (docs/modes.md section 4n).  feat: NHWC [2N, H, W, C], entries 0 .. N-1 the features of
    image a and N .. 2N-1 those of image b; w: [C], the layer's "lin" weights -> device double [N], the mean over the pixels of
    sum_c w_c (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2; with return_map also the [N, H, W] double map.  Like every NHWC op
    here it takes contiguous tensors only (_chk): a view raises."""
    _chk(feat, "lpips_layer.feat")
    _chk(w, "lpips_layer.w")
    if feat.dim() != 4 or feat.shape[0] < 2 or feat.shape[0] % 2:
        raise _lib.PesrHipError(f"lpips_layer: expected a [2N, H, W, C] tensor (a's features, then b's), got {tuple(feat.shape)}")
    N, H, W, C = feat.shape[0] // 2, feat.shape[1], feat.shape[2], feat.shape[3]
    if w.dim() != 1 or w.shape[0] != C:
        raise _lib.PesrHipError(f"lpips_layer: expected {C} weights, got {tuple(w.shape)}")
    out = torch.empty(N, dtype=torch.float64, device=feat.device)
    dmap = torch.empty((N, H, W), dtype=torch.float64, device=feat.device) if return_map else None
    ws = workspace(8 * N * ((H * W + 63) // 64), feat.device)
    rc = _lib.lib().pesr_lpips_layer(_p(feat), _p(w), _p(out), N, H, W, C, _p(dmap), _p(ws), ws.numel(), _stream())
    _lib.check(rc, "pesr_lpips_layer")
    return (out, dmap) if return_map else out


def _chk_lpips_pair(what: str, fa: torch.Tensor, fb: torch.Tensor, w: torch.Tensor):
    _chk(fa, f"{what}.fa")
    _chk(fb, f"{what}.fb")
    _chk(w, f"{what}.w")
    if fa.dim() != 4 or fa.shape[0] < 1 or tuple(fb.shape) != tuple(fa.shape):
        raise _lib.PesrHipError(f"{what}: expected two [N, H, W, C] tensors of one shape, got {tuple(fa.shape)} and {tuple(fb.shape)}")
    if w.dim() != 1 or w.shape[0] != fa.shape[3]:
        raise _lib.PesrHipError(f"{what}: expected {fa.shape[3]} weights, got {tuple(w.shape)}")
    return tuple(fa.shape)


def lpips_layer_pair(fa: torch.Tensor, fb: torch.Tensor, w: torch.Tensor, return_map: bool = False):
    """lpips_layer with the two feature tensors apart: fa, fb NHWC [N, H, W, C] each (docs/modes.md section 4o) -> what
    lpips_layer(cat([fa, fb]), w, return_map) gives, bit for bit (one kernel), without the cat."""
    N, H, W, C = _chk_lpips_pair("lpips_layer_pair", fa, fb, w)
    out = torch.empty(N, dtype=torch.float64, device=fa.device)
    dmap = torch.empty((N, H, W), dtype=torch.float64, device=fa.device) if return_map else None
    ws = workspace(8 * N * ((H * W + 63) // 64), fa.device)
    rc = _lib.lib().pesr_lpips_layer2(_p(fa), _p(fb), _p(w), _p(out), N, H, W, C, _p(dmap), _p(ws), ws.numel(), _stream())
    _lib.check(rc, "pesr_lpips_layer2")
    return (out, dmap) if return_map else out


def lpips_layer_bwd(fa: torch.Tensor, fb: torch.Tensor, w: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """The gradient of lpips_layer_pair(fa, fb, w) with respect to fa (docs/modes.md section 4o).  g: device double [N], dL/dscore of
    each pair -> fp32 [N, H, W, C]: (2 g[n] / (H W)) (w_j t_j - (a_j / na) q) / (na + 1e-10) with q = sum_c w_c t_c ah_c, and 0 at every
    pixel whose fa vector is all zero (na == 0: a definition, the formula's value there is 2 w_j t_j / 1e-10).  fb gets none."""
    N, H, W, C = _chk_lpips_pair("lpips_layer_bwd", fa, fb, w)
    if not g.is_cuda or g.dtype != torch.float64 or tuple(g.shape) != (N,) or not g.is_contiguous():
        raise _lib.PesrHipError(f"lpips_layer_bwd.g: expected a contiguous float64 GPU tensor [{N}], got {g.dtype} {tuple(g.shape)}")
    ga = torch.empty((N, H, W, C), dtype=torch.float32, device=fa.device)
    rc = _lib.lib().pesr_lpips_layer_bwd(_p(fa), _p(fb), _p(w), _p(g), _p(ga), N, H, W, C, _stream())
    _lib.check(rc, "pesr_lpips_layer_bwd")
    return ga


# ------------------------------------------------------------------------------------------------
# DISTS (docs/modes.md section 4t): the trunk's L2 pooling and the head of one stage (pesr_amd/csrc/dists.hip)
# ------------------------------------------------------------------------------------------------
DISTS_CHANNELS = (3, 64, 128, 256, 512)


def l2pool_plan(N: int, H: int, W: int, C: int) -> dict:
    """What l2pool_fwd does with an NHWC [N, H, W, C] input (a host-only question): {"blocks": its workgroups, "floats_per_block": the
    output elements one workgroup writes, 1024 / C pixels}.  ValueError for a shape the kernel does not take."""
    blocks = _memo("pesr_l2pool_blocks", N, H, W, C)
    if blocks < 1:
        raise ValueError(f"l2pool_plan: no L2 pooling kernel for N {N}, H {H}, W {W}, C {C}")
    return {"blocks": blocks, "floats_per_block": 1024}


def l2pool_fwd(x: torch.Tensor) -> torch.Tensor:
    """DISTS's L2 pooling.  x: NHWC [N, H, W, C], C a multiple of 64 -> [N, ceil(H/2), ceil(W/2), C] =
    sqrt(conv(x * x, [1,2,1] (x) [1,2,1] / 16, stride 2, zero padding 1, depthwise) + 1e-12).  Forward only."""
    _chk(x, "l2pool_fwd.x")
    if x.dim() != 4 or min(x.shape) < 1:
        raise _lib.PesrHipError(f"l2pool_fwd.x: expected a [N, H, W, C] tensor, got {tuple(x.shape)}")
    N, H, W, C = x.shape
    if C % 64:
        raise _lib.PesrHipError(f"l2pool_fwd.x: C = {C}, the L2 pooling kernel takes multiples of 64")
    y = torch.empty((N, (H + 1) // 2, (W + 1) // 2, C), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().pesr_l2pool_fwd(_p(x), _p(y), N, H, W, C, _stream()), "pesr_l2pool_fwd")
    return y


def dists_plan(N: int, P: int, C: int) -> dict:
    """What dists_layer does with N image pairs of P pixels and C channels (a host-only question): {"pixel_blocks": the blocks of
    pixels_per_block = 256 pixels whose partial sums are combined in ascending order; "workspace_bytes"}.  ValueError for a shape the
    kernels do not take."""
    nb = _memo("pesr_dists_pixel_blocks", N, P, C)
    if nb < 1:
        raise ValueError(f"dists_plan: no DISTS head kernel for N {N}, P {P}, C {C}")
    return {"pixel_blocks": nb, "pixels_per_block": 256, "workspace_bytes": int(_lib.lib().pesr_dists_workspace_bytes(N, P, C))}


def _chk_dists_weights(name: str, t, C: int):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.PesrHipError(f"dists_layer.{name}: pesr_amd ops run only on a GPU (HIP) tensor; there is no CPU fallback")
    if t.dtype != torch.float64:
        raise _lib.PesrHipError(f"dists_layer.{name}: expected float64, got {t.dtype}")
    if t.dim() != 1 or t.shape[0] != C:
        raise _lib.PesrHipError(f"dists_layer.{name}: expected {C} weights, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise _lib.PesrHipError(f"dists_layer.{name}: expected a contiguous tensor")


def dists_layer(feat: torch.Tensor, alpha: torch.Tensor, beta: torch.Tensor, return_stats: bool = False):
    """The DISTS head of one stage (docs/modes.md section 4t).  feat: NHWC [2N, H, W, C], entries 0 .. N-1 the features of image a and
    N .. 2N-1 those of image b, C in DISTS_CHANNELS (3: the image itself); alpha, beta: float64 [C], the stage's slices of alpha / w and
    beta / w -> device double [N], sum_c alpha_c S1_c + beta_c S2_c; with return_stats also the [N, C, 5] doubles (mu_a, mu_b, var_a,
    var_b, cov).  Contiguous tensors only (_chk): a view raises."""
    _chk(feat, "dists_layer.feat")
    if feat.dim() != 4 or feat.shape[0] < 2 or feat.shape[0] % 2 or min(feat.shape) < 1:
        raise _lib.PesrHipError(f"dists_layer.feat: expected a [2N, H, W, C] tensor (a's features, then b's), got {tuple(feat.shape)}")
    N, H, W, C = feat.shape[0] // 2, feat.shape[1], feat.shape[2], feat.shape[3]
    if C not in DISTS_CHANNELS:
        raise _lib.PesrHipError(f"dists_layer.feat: C = {C}, the DISTS head takes C in {DISTS_CHANNELS}")
    _chk_dists_weights("alpha", alpha, C)
    _chk_dists_weights("beta", beta, C)
    out = torch.empty(N, dtype=torch.float64, device=feat.device)
    stats = torch.empty((N, C, 5), dtype=torch.float64, device=feat.device) if return_stats else None
    ws = workspace(int(_lib.lib().pesr_dists_workspace_bytes(N, H * W, C)), feat.device)
    rc = _lib.lib().pesr_dists_layer(_p(feat), _p(alpha), _p(beta), _p(out), N, H, W, C, _p(stats), _p(ws), ws.numel(), _stream())
    _lib.check(rc, "pesr_dists_layer")
    return (out, stats) if return_stats else out


# ------------------------------------------------------------------------------------------------
# channel attention of a residual block (docs/modes.md section 4u; pesr_amd/csrc/channel_attention.hip).  fp32 whatever PRECISION is.
# ------------------------------------------------------------------------------------------------
CA_MAX_CHANNELS = 2048


def ca_check_channels(what: str, n_feats: int, reduction: int) -> int:
    """-> R = n_feats / reduction, the hidden units of the gate; ValueError naming the argument the kernels cannot take."""
    if n_feats < 4 or n_feats % 4 or n_feats > CA_MAX_CHANNELS:
        raise ValueError(f"{what}: n_feats = {n_feats}; the channel-attention kernels take a multiple of 4 up to {CA_MAX_CHANNELS}")
    if reduction < 1 or n_feats % reduction:
        raise ValueError(f"{what}: reduction = {reduction}; it has to be >= 1 and divide n_feats = {n_feats}")
    return n_feats // reduction


def ca_pool_partials(N: int, HW: int, C: int) -> int:
    """The chunks an image's HW pixels are cut into by the two pixel sums (ca_pool, ca_ds) - one workgroup and one partial row each,
    combined in ascending order (a host-only question).  ValueError for a shape the kernels do not take."""
    if C < 4 or C % 4 or C > CA_MAX_CHANNELS:
        raise ValueError(f"ca_pool_partials: C = {C}; the channel-attention kernels take a multiple of 4 up to {CA_MAX_CHANNELS}")
    if N < 1:
        raise ValueError(f"ca_pool_partials: N = {N}")
    if HW < 1 or HW > 1 << 30:
        raise ValueError(f"ca_pool_partials: HW = {HW}")
    return _memo("pesr_ca_pool_partials", N, HW, C)


def _ca_map(what: str, t: torch.Tensor):
    _chk(t, what)
    if t.dim() != 4 or min(t.shape) < 1:
        raise ValueError(f"{what}: expected a [N, H, W, C] tensor, got {tuple(t.shape)}")
    N, H, W, C = t.shape
    ca_pool_partials(N, H * W, C)
    return N, H * W, C


def _ca_mat(what: str, t: torch.Tensor, shape) -> torch.Tensor:
    """A gate tensor ([N, C] / [N, R] / a 1 x 1 conv's weight or bias) as the contiguous fp32 matrix the kernels read."""
    _chk(t, what)
    if t.numel() != shape[0] * shape[1] or t.shape[0] != shape[0]:
        raise ValueError(f"{what}: expected {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _ca_ws(N: int, HW: int, C: int, R: int, device):
    return workspace(int(_lib.lib().pesr_ca_workspace_bytes(N, HW, C, R)), device)


def ca_pool(t: torch.Tensor) -> torch.Tensor:
    """t: NHWC [N, H, W, C] -> m [N, C], the mean over the pixels (fp32 partial sums per chunk, combined in double in a fixed order)."""
    N, HW, C = _ca_map("ca_pool.t", t)
    m = torch.empty((N, C), dtype=torch.float32, device=t.device)
    ws = _ca_ws(N, HW, C, 1, t.device)
    _lib.check(_lib.lib().pesr_ca_pool(_p(t), _p(m), N, HW, C, _p(ws), ws.numel(), _stream()), "pesr_ca_pool")
    return m


def ca_ds(gy: torch.Tensor, t: torch.Tensor, res_scale: float) -> torch.Tensor:
    """-> ds [N, C] = res_scale * sum over the pixels of gy * t (the gradient of the gate's output s)."""
    N, HW, C = _ca_map("ca_ds.t", t)
    _chk(gy, "ca_ds.gy")
    if gy.shape != t.shape:
        raise ValueError(f"ca_ds.gy: expected {tuple(t.shape)}, got {tuple(gy.shape)}")
    ds = torch.empty((N, C), dtype=torch.float32, device=t.device)
    ws = _ca_ws(N, HW, C, 1, t.device)
    _lib.check(_lib.lib().pesr_ca_ds(_p(gy), _p(t), _p(ds), N, HW, C, float(res_scale), _p(ws), ws.numel(), _stream()), "pesr_ca_ds")
    return ds


def ca_gate_fwd(m: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor):
    """m [N, C]; w1 [R, C(, 1, 1)], b1 [R], w2 [C, R(, 1, 1)], b2 [C] -> (h [N, R] = relu(w1 m + b1), s [N, C] = sigmoid(w2 h + b2))."""
    _chk(m, "ca_gate_fwd.m")
    if m.dim() != 2:
        raise ValueError(f"ca_gate_fwd.m: expected [N, C], got {tuple(m.shape)}")
    N, C = m.shape
    R = w1.shape[0]
    ca_check_channels("ca_gate_fwd", C, C // R if R and C % R == 0 else 0)
    _ca_mat("ca_gate_fwd.w1", w1, (R, C)), _ca_mat("ca_gate_fwd.b1", b1, (R, 1))
    _ca_mat("ca_gate_fwd.w2", w2, (C, R)), _ca_mat("ca_gate_fwd.b2", b2, (C, 1))
    h = torch.empty((N, R), dtype=torch.float32, device=m.device)
    s = torch.empty((N, C), dtype=torch.float32, device=m.device)
    _lib.check(_lib.lib().pesr_ca_gate_fwd(_p(m), _p(w1), _p(b1), _p(w2), _p(b2), _p(h), _p(s), N, C, R, _stream()), "pesr_ca_gate_fwd")
    return h, s


def ca_apply_fwd(x: torch.Tensor, t: torch.Tensor, s: torch.Tensor, res_scale: float) -> torch.Tensor:
    """y = x + res_scale * t * s[n, c];  x, t: NHWC [N, H, W, C], s [N, C]."""
    N, HW, C = _ca_map("ca_apply_fwd.t", t)
    _chk(x, "ca_apply_fwd.x")
    if x.shape != t.shape:
        raise ValueError(f"ca_apply_fwd.x: expected {tuple(t.shape)}, got {tuple(x.shape)}")
    _ca_mat("ca_apply_fwd.s", s, (N, C))
    y = torch.empty_like(t)
    _lib.check(_lib.lib().pesr_ca_apply_fwd(_p(x), _p(t), _p(s), _p(y), N, HW, C, float(res_scale), _stream()), "pesr_ca_apply_fwd")
    return y


def ca_gate_bwd(ds, s, h, m, w1, w2, dw1_out=None, db1_out=None, dw2_out=None, db2_out=None):
    """The gate's backward: ds, s, m [N, C], h [N, R], w1 [R, C(, 1, 1)], w2 [C, R(, 1, 1)] -> (dm [N, C], dw1, db1, dw2, db2), the
    parameter gradients summed over the batch in increasing n, shaped like w1, [R], like w2, [C]; *_out: where to write them."""
    _chk(ds, "ca_gate_bwd.ds")
    if ds.dim() != 2:
        raise ValueError(f"ca_gate_bwd.ds: expected [N, C], got {tuple(ds.shape)}")
    N, C = ds.shape
    R = w1.shape[0]
    ca_check_channels("ca_gate_bwd", C, C // R if R and C % R == 0 else 0)
    for name, t, shape in (("s", s, (N, C)), ("h", h, (N, R)), ("m", m, (N, C)), ("w1", w1, (R, C)), ("w2", w2, (C, R))):
        _ca_mat("ca_gate_bwd." + name, t, shape)
    dev = ds.device
    dm = torch.empty((N, C), dtype=torch.float32, device=dev)
    dw1, db1 = _out(dw1_out, w1.shape, dev), _out(db1_out, (R,), dev)
    dw2, db2 = _out(dw2_out, w2.shape, dev), _out(db2_out, (C,), dev)
    ws = _ca_ws(N, 1, C, R, dev)
    rc = _lib.lib().pesr_ca_gate_bwd(_p(ds), _p(s), _p(h), _p(m), _p(w1), _p(w2), _p(dm), _p(dw1), _p(db1), _p(dw2), _p(db2), N, C, R,
                                     _p(ws), ws.numel(), _stream())
    _lib.check(rc, "pesr_ca_gate_bwd")
    return dm, dw1, db1, dw2, db2


def ca_apply_bwd(gy: torch.Tensor, s: torch.Tensor, dm: torch.Tensor, res_scale: float) -> torch.Tensor:
    """gt = res_scale * gy * s[n, c] + dm[n, c] / HW;  gy: NHWC [N, H, W, C], s, dm [N, C]."""
    N, HW, C = _ca_map("ca_apply_bwd.gy", gy)
    _ca_mat("ca_apply_bwd.s", s, (N, C)), _ca_mat("ca_apply_bwd.dm", dm, (N, C))
    gt = torch.empty_like(gy)
    _lib.check(_lib.lib().pesr_ca_apply_bwd(_p(gy), _p(s), _p(dm), _p(gt), N, HW, C, float(res_scale), _stream()), "pesr_ca_apply_bwd")
    return gt


# ------------------------------------------------------------------------------------------------
# the U-Net discriminator's own kernels (docs/modes.md section 4v): bilinear x2 (csrc/upsample2x.hip), the 3 x 3 conv to one channel
# (csrc/conv_c1.hip); the GAN loss of a logit map stands with gan_loss at the end of this file.  fp32 whatever PRECISION is.
# ------------------------------------------------------------------------------------------------
def _up2_map(what: str, t: torch.Tensor):
    _chk(t, what)
    if t.dim() != 4 or min(t.shape) < 1:
        raise ValueError(f"{what}: expected a [N, H, W, C] tensor with no empty axis, got {tuple(t.shape)}")
    return tuple(t.shape)


def bilinear_up2_fwd(a: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a (and b, same shape): NHWC [N, H, W, C] -> [N, 2H, 2W, C] = up2(a + b), up2 = F.interpolate(scale_factor=2, mode='bilinear',
    align_corners=False); a + b is rounded once, as torch's own addition would."""
    N, H, W, C = _up2_map("bilinear_up2_fwd.a", a)
    if b is not None:
        _chk(b, "bilinear_up2_fwd.b")
        if b.shape != a.shape:
            raise ValueError(f"bilinear_up2_fwd.b: expected {tuple(a.shape)}, got {tuple(b.shape)}")
    y = torch.empty((N, 2 * H, 2 * W, C), dtype=torch.float32, device=a.device)
    rc = _lib.lib().pesr_bilinear_up2_fwd(_p(a), _p(b), _p(y), N, H, W, C, _stream())
    if rc == -1:
        raise ValueError(f"bilinear_up2_fwd.a: shape {(N, H, W, C)} is beyond what the kernel indexes")
    _lib.check(rc, f"pesr_bilinear_up2_fwd[{N}x{H}x{W}x{C}]")
    return y


def bilinear_up2_bwd(gy: torch.Tensor) -> torch.Tensor:
    """gy: NHWC [N, 2H, 2W, C] -> gx [N, H, W, C], the adjoint of bilinear_up2_fwd (the gradient of a, and of b)."""
    N, H2, W2, C = _up2_map("bilinear_up2_bwd.gy", gy)
    if H2 % 2 or W2 % 2:
        raise ValueError(f"bilinear_up2_bwd.gy: expected even height and width, got {tuple(gy.shape)}")
    gx = torch.empty((N, H2 // 2, W2 // 2, C), dtype=torch.float32, device=gy.device)
    rc = _lib.lib().pesr_bilinear_up2_bwd(_p(gy), _p(gx), N, H2 // 2, W2 // 2, C, _stream())
    if rc == -1:
        raise ValueError(f"bilinear_up2_bwd.gy: shape {tuple(gy.shape)} is beyond what the kernel indexes")
    _lib.check(rc, f"pesr_bilinear_up2_bwd[{N}x{H2 // 2}x{W2 // 2}x{C}]")
    return gx


C1_MAX_CHANNELS = 1024


def c1_eligible(cin: int, cout: int, stride: int) -> bool:
    """Shapes of the pesr_conv3x3_c1_* kernels (C -> 1, stride 1): the implicit-GEMM kernels take no one-channel gradient."""
    return cout == 1 and stride == 1 and cin % 4 == 0 and 4 <= cin <= C1_MAX_CHANNELS


def _c1_pair(what: str, x_shape, x: Optional[torch.Tensor], dy: Optional[torch.Tensor], w: Optional[torch.Tensor]):
    N, H, W, C = x_shape
    if not c1_eligible(C, 1, 1) or N < 1 or H < 1 or W < 1 or N * H * W >= 1 << 31:
        raise ValueError(f"{what}.x: shape {tuple(x_shape)}; the C -> 1 kernels take a multiple of 4 channels up to {C1_MAX_CHANNELS} and "
                         f"fewer than 2^31 pixels")
    for name, t, shape in (("x", x, (N, H, W, C)), ("dy", dy, (N, H, W, 1)), ("w", w, (1, C, 3, 3))):
        if t is not None:
            _chk(t, f"{what}.{name}")
            if tuple(t.shape) != shape:
                raise ValueError(f"{what}.{name}: expected {shape}, got {tuple(t.shape)}")
    return N, H, W, C


def conv3x3_c1_fwd(x: torch.Tensor, w_oihw: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """y [N, H, W, 1] = conv(x [N, H, W, C], w OIHW [1, C, 3, 3]) + bias [1]."""
    N, H, W, C = _c1_pair("conv3x3_c1_fwd", x.shape, x, None, w_oihw)
    y = torch.empty((N, H, W, 1), dtype=torch.float32, device=x.device)
    _conv_flops(N, H, W, C, 1, _RGB_VALU)
    br = OP_EVENTS.begin(f"conv_c1 {C}->1")
    rc = _lib.lib().pesr_conv3x3_c1_fwd(_p(x), _p(w_oihw), _p(bias), _p(y), N, H, W, C, _stream())
    OP_EVENTS.end(br)
    _lib.check(rc, f"pesr_conv3x3_c1_fwd[{N}x{H}x{W}x{C}->1]")
    return y


def conv3x3_c1_dgrad(dy: torch.Tensor, w_oihw: torch.Tensor, in_shape) -> torch.Tensor:
    """dx [N, H, W, C] of that conv from dy [N, H, W, 1]."""
    N, H, W, C = _c1_pair("conv3x3_c1_dgrad", tuple(in_shape), None, dy, w_oihw)
    dx = torch.empty((N, H, W, C), dtype=torch.float32, device=dy.device)
    _conv_flops(N, H, W, C, 1, _RGB_VALU)
    rc = _lib.lib().pesr_conv3x3_c1_dgrad(_p(dy), _p(w_oihw), _p(dx), N, H, W, C, _stream())
    _lib.check(rc, f"pesr_conv3x3_c1_dgrad[{N}x{H}x{W}x{C}<-1]")
    return dx


def conv3x3_c1_wgrad(x: torch.Tensor, dy: torch.Tensor, alpha: float = 1.0, want_bias: bool = True, dw_out=None, db_out=None):
    """(dw [1, C, 3, 3], db [1] | None) of that conv: per-chunk fp32 rows, added in double in a fixed order."""
    N, H, W, C = _c1_pair("conv3x3_c1_wgrad", x.shape, x, dy, None)
    L = _lib.lib()
    ws = workspace(int(L.pesr_conv3x3_c1_wgrad_workspace_bytes(N, H, W, C)), x.device)
    dw = _out(dw_out, (1, C, 3, 3), x.device)
    db = _out(db_out, (1,), x.device) if want_bias else None
    _conv_flops(N, H, W, C, 1, _RGB_VALU)
    rc = L.pesr_conv3x3_c1_wgrad(_p(x), _p(dy), _p(dw), _p(db), N, H, W, C, float(alpha), _p(ws), ws.numel(), _stream())
    _lib.check(rc, f"pesr_conv3x3_c1_wgrad[{N}x{H}x{W}x{C}->1]")
    return dw, db


# ------------------------------------------------------------------------------------------------
# window self-attention of the Generator's attention blocks (docs/modes.md section 4w; pesr_amd/csrc/window_attention.hip).  fp32
# whatever PRECISION is.
# ------------------------------------------------------------------------------------------------
WATTN_WINDOW = 8          # pixels per window side
WATTN_HEAD = 32           # channels per head; tau = 1 / sqrt(WATTN_HEAD) is the kernels'
WATTN_MAX_DIM = 1024      # the kernels' cap on the attention width


def routed_3x3_width_ok(c: int) -> bool:
    """A channel count that the routed 3 x 3 path takes on either side of a conv in all three passes: the forward wants Cin % 16 == 0
    (it pads Cout to its tile itself), the input gradient is the same kernel with the two exchanged, so Cout % 16 == 0; the weight
    gradient wants multiples of 4 (tests/test_window_attention_cpu.py asks the library)."""
    return c >= 16 and c % 16 == 0


def wattn_check_widths(what: str, n_feats: int, dim: int) -> int:
    """-> the heads of an attention block of width dim on n_feats features; ValueError naming the argument that cannot be taken.  (A
    multiple of 32 and its threefold are multiples of 16: every legal dim suits the projections n_feats -> 3 dim and dim -> n_feats.)"""
    if dim < WATTN_HEAD or dim % WATTN_HEAD or dim > WATTN_MAX_DIM:
        raise ValueError(f"{what}: dim = {dim}; the attention width has to be a multiple of {WATTN_HEAD} (the head width) from "
                         f"{WATTN_HEAD} to {WATTN_MAX_DIM}")
    if not routed_3x3_width_ok(n_feats):
        raise ValueError(f"{what}: n_feats = {n_feats}; the 3 x 3 conv kernels take the block's projections forward and backward only "
                         f"where n_feats is a multiple of 16")
    return dim // WATTN_HEAD


def _wattn_shape(what: str, qkv: torch.Tensor, shift: int):
    _chk(qkv, what)
    if qkv.dim() != 4 or min(qkv.shape) < 1 or qkv.shape[3] % (3 * WATTN_HEAD) or qkv.shape[3] > 3 * WATTN_MAX_DIM:
        raise ValueError(f"{what}: expected [N, H, W, 3 D] with D a multiple of {WATTN_HEAD} up to {WATTN_MAX_DIM}, got {tuple(qkv.shape)}")
    if not 0 <= shift < WATTN_WINDOW:
        raise ValueError(f"{what}: shift = {shift}; expected 0 .. {WATTN_WINDOW - 1}")
    N, H, W, D3 = qkv.shape
    return N, H, W, D3 // 3


def window_attention_fwd(qkv: torch.Tensor, shift: int = 0) -> torch.Tensor:
    """qkv: NHWC [N, H, W, 3 D] (q | k | v, heads of 32 channels) -> out [N, H, W, D]: softmax(q k^T / sqrt(32)) v per 8 x 8 window of the
    grid with its origin at (-shift, -shift) and per head, over the window's pixels inside the image."""
    N, H, W, D = _wattn_shape("window_attention_fwd.qkv", qkv, shift)
    out = torch.empty((N, H, W, D), dtype=torch.float32, device=qkv.device)
    _lib.check(_lib.lib().pesr_window_attention_fwd(_p(qkv), _p(out), N, H, W, D, int(shift), _stream()), "pesr_window_attention_fwd")
    return out


def window_attention_bwd(qkv: torch.Tensor, dout: torch.Tensor, shift: int = 0) -> torch.Tensor:
    """-> dqkv [N, H, W, 3 D], the gradient of window_attention_fwd's input for the gradient dout [N, H, W, D] of its output (the attention
    matrix is recomputed from qkv)."""
    N, H, W, D = _wattn_shape("window_attention_bwd.qkv", qkv, shift)
    _chk(dout, "window_attention_bwd.dout")
    if tuple(dout.shape) != (N, H, W, D):
        raise ValueError(f"window_attention_bwd.dout: expected {(N, H, W, D)}, got {tuple(dout.shape)}")
    dqkv = torch.empty_like(qkv)
    _lib.check(_lib.lib().pesr_window_attention_bwd(_p(qkv), _p(dout), _p(dqkv), N, H, W, D, int(shift), _stream()),
               "pesr_window_attention_bwd")
    return dqkv


# ------------------------------------------------------------------------------------------------
# LayerNorm over the channels of each pixel, in front of the window attention (docs/modes.md section 4x; pesr_amd/csrc/layernorm.hip).
# fp32 whatever PRECISION is.
# ------------------------------------------------------------------------------------------------
LN_EPS = 1e-5
LN_MAX_CHANNELS = 1024    # the kernels' cap on C
_LN_LANES = 256           # of a workgroup


def ln_check_channels(what: str, C: int) -> None:
    if C < 4 or C % 4 or C > LN_MAX_CHANNELS:
        raise ValueError(f"{what}: C = {C}; the LayerNorm kernels take a multiple of 4 from 4 to {LN_MAX_CHANNELS}")


def layernorm_partials(P: int, C: int) -> int:
    """The workgroups of a LayerNorm launch over P pixels of C channels = the partial rows of the backward's channel sums, combined in
    ascending order (a host-only question; a function of the shape alone).  ValueError for a shape the kernels do not take."""
    ln_check_channels("layernorm_partials", C)
    if P < 1:
        raise ValueError(f"layernorm_partials: P = {P}")
    return _memo("pesr_layernorm_partials", P, C)


def layernorm_pass_pixels(P: int, C: int) -> int:
    """The pixels one step of the whole grid covers: with more than these a workgroup walks on (csrc/layernorm.hip: a group of G lanes per
    pixel, G the power of two that covers C / 4 up to 64; 4, 2, 1, 1 pixels per group and step at 1, 2, 3, 4 pieces per lane)."""
    group = 1
    while group < C // 4 and group < 64:
        group *= 2
    pieces = (C // 4 + 63) // 64
    return layernorm_partials(P, C) * (_LN_LANES // group) * (4, 2, 1, 1)[pieces - 1]


def _ln_rows(what: str, x: torch.Tensor):
    _chk(x, what)
    if x.dim() < 2 or min(x.shape) < 1:
        raise ValueError(f"{what}: expected [..., C] with at least one pixel, got {tuple(x.shape)}")
    C = x.shape[-1]
    ln_check_channels(what, C)
    return x.numel() // C, C


def _ln_vec(what: str, t: torch.Tensor, C: int) -> None:
    _chk(t, what)
    if tuple(t.shape) != (C,):
        raise ValueError(f"{what}: expected {(C,)}, got {tuple(t.shape)}")


def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor):
    """x: [..., C] (NHWC: every pixel on its own) -> (y, stats): y = (x - mean) * rstd * gamma + beta over the channels of each pixel
    with the centred variance and eps = LN_EPS; stats [P, 2] = (mean, rstd) is what layernorm_bwd wants back."""
    P, C = _ln_rows("layernorm_fwd.x", x)
    _ln_vec("layernorm_fwd.gamma", gamma, C)
    _ln_vec("layernorm_fwd.beta", beta, C)
    y = torch.empty_like(x)
    stats = torch.empty((P, 2), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().pesr_layernorm_fwd(_p(x), _p(gamma), _p(beta), _p(y), _p(stats), P, C, LN_EPS, _stream()), "pesr_layernorm_fwd")
    return y, stats


def layernorm_bwd(x: torch.Tensor, gamma: torch.Tensor, stats: torch.Tensor, dy: torch.Tensor, dgamma_out=None, dbeta_out=None):
    """-> (dx, dgamma, dbeta) of layernorm_fwd for the gradient dy of its output; every element written once, the channel sums through
    per-workgroup partial rows in the pooled workspace, added in double in a fixed order.  dgamma_out / dbeta_out: a parameter's
    flat-gradient view to write into."""
    P, C = _ln_rows("layernorm_bwd.x", x)
    _ln_vec("layernorm_bwd.gamma", gamma, C)
    _chk(stats, "layernorm_bwd.stats")
    _chk(dy, "layernorm_bwd.dy")
    if tuple(stats.shape) != (P, 2):
        raise ValueError(f"layernorm_bwd.stats: expected {(P, 2)}, got {tuple(stats.shape)}")
    if dy.shape != x.shape:
        raise ValueError(f"layernorm_bwd.dy: expected {tuple(x.shape)}, got {tuple(dy.shape)}")
    dx = torch.empty_like(x)
    dgamma, dbeta = _out(dgamma_out, (C,), x.device), _out(dbeta_out, (C,), x.device)
    ws = workspace(int(_lib.lib().pesr_layernorm_workspace_bytes(P, C)), x.device)
    _lib.check(_lib.lib().pesr_layernorm_bwd(_p(x), _p(gamma), _p(stats), _p(dy), _p(dx), _p(dgamma), _p(dbeta), _p(ws), P, C, _stream()),
               "pesr_layernorm_bwd")
    return dx, dgamma, dbeta


# ------------------------------------------------------------------------------------------------
# texture loss: patch-wise Gram matrices (docs/modes.md section 4q)
# ------------------------------------------------------------------------------------------------
GRAM_CHANNELS = (64, 128, 256)


def _gram_patch(what: str, H: int, W: int, patch):
    """patch: 0 (the whole map), a side, or (ph, pw) -> (ph, pw); PesrHipError unless it tiles the H x W map."""
    ph, pw = (patch, patch) if isinstance(patch, int) else (int(patch[0]), int(patch[1]))
    ph, pw = (ph or H), (pw or W)
    if ph < 1 or pw < 1 or H % ph or W % pw:
        raise _lib.PesrHipError(f"{what}: a {ph} x {pw} patch does not tile a {H} x {W} map")
    return ph, pw


def _chk_gram_feat(what: str, f: torch.Tensor):
    if not torch.is_tensor(f) or not f.is_cuda or f.dtype != torch.float32 or f.dim() != 4 or not f.is_contiguous() or f.shape[0] < 1:
        raise _lib.PesrHipError(f"{what}: expected contiguous [N, H, W, C] float32 GPU tensors (NHWC features; there is no CPU path)")
    if f.shape[3] not in GRAM_CHANNELS:
        raise _lib.PesrHipError(f"{what}: C = {f.shape[3]}, the Gram kernels take C in {GRAM_CHANNELS}")
    return tuple(f.shape)


def gram_plan(N: int, H: int, W: int, C: int, ph: int, pw: int) -> dict:
    """What pesr_gram_fwd does with this shape (a host-only question): {"splits": the number of K slices, 1 = the kernel writes G
    itself; "workspace_bytes": the partial sums' slabs, 0 without a split; "patches": P; "pixels": K}.  ValueError for a shape the
    kernels do not take."""
    s = _memo("pesr_gram_splits", N, H, W, C, ph, pw)
    if s < 1:
        raise ValueError(f"gram_plan: no Gram kernel for N {N}, {H} x {W} x {C}, patch {ph} x {pw}")
    return {"splits": s, "workspace_bytes": int(_lib.lib().pesr_gram_workspace_bytes(N, H, W, C, ph, pw)),
            "patches": (H // ph) * (W // pw), "pixels": ph * pw}


def gram(f: torch.Tensor, patch=0) -> torch.Tensor:
    """Patch-wise Gram matrices of NHWC features f [N, H, W, C] (C in GRAM_CHANNELS): fp32 [N, P, C, C],
    G[n, p] = F_p^T F_p / (C K) over the K pixels of patch p, on the fp32 MFMA; bit-for-bit symmetric and reproducible.  patch: 0 = the
    whole map, a side, or (ph, pw); it must tile the map."""
    N, H, W, C = _chk_gram_feat("gram", f)
    ph, pw = _gram_patch("gram", H, W, patch)
    plan = gram_plan(N, H, W, C, ph, pw)
    G = torch.empty((N, plan["patches"], C, C), dtype=torch.float32, device=f.device)
    ws = workspace(plan["workspace_bytes"], f.device)
    rc = _lib.lib().pesr_gram_fwd(_p(f), _p(G), N, H, W, C, ph, pw, _p(ws), ws.numel(), _stream())
    _lib.check(rc, "pesr_gram_fwd")
    return G


def gram_loss(ga: torch.Tensor, gb: torch.Tensor, need_grad: bool = False):
    """(ga, gb) fp32 [N, P, C, C] -> (device double [N]: sum over patches and entries of (ga - gb)^2, divided by P, the difference
    taken in double; dG).  dG is None unless need_grad: then fp32 [N, P, C, C], the difference rounded once, what gram_bwd reads."""
    for t in (ga, gb):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous() \
                or t.shape[0] < 1 or t.shape[2] != t.shape[3]:
            raise _lib.PesrHipError("gram_loss: expected contiguous [N, P, C, C] float32 GPU tensors (there is no CPU path)")
    if tuple(ga.shape) != tuple(gb.shape):
        raise _lib.PesrHipError(f"gram_loss: the two tensors differ in shape: {tuple(ga.shape)} and {tuple(gb.shape)}")
    N, P, C = ga.shape[0], ga.shape[1], ga.shape[2]
    if C not in GRAM_CHANNELS:
        raise _lib.PesrHipError(f"gram_loss: C = {C}, the Gram kernels take C in {GRAM_CHANNELS}")
    t = torch.empty(N, dtype=torch.float64, device=ga.device)
    dg = torch.empty_like(ga) if need_grad else None
    ws = workspace(int(_lib.lib().pesr_gram_loss_workspace_bytes(N, P, C)), ga.device)
    rc = _lib.lib().pesr_gram_loss(_p(ga), _p(gb), _p(t), _p(dg), N, P, C, _p(ws), ws.numel(), _stream())
    _lib.check(rc, "pesr_gram_loss")
    return t, dg


def gram_bwd(f: torch.Tensor, dg: torch.Tensor, g: torch.Tensor, patch=0) -> torch.Tensor:
    """The gradient of sum_n g[n] t[n] (gram_loss of gram(f, patch) against anything) with respect to f: fp32 [N, H, W, C],
    g[n] (4 / (C K P)) F dG per patch.  dg: gram_loss's symmetric fp32 [N, P, C, C]; g: device double [N].  Not masked by f > 0."""
    N, H, W, C = _chk_gram_feat("gram_bwd", f)
    ph, pw = _gram_patch("gram_bwd", H, W, patch)
    P = (H // ph) * (W // pw)
    if not torch.is_tensor(dg) or not dg.is_cuda or dg.dtype != torch.float32 or tuple(dg.shape) != (N, P, C, C) or not dg.is_contiguous():
        raise _lib.PesrHipError(f"gram_bwd.dg: expected a contiguous float32 GPU tensor [{N}, {P}, {C}, {C}]")
    if not torch.is_tensor(g) or not g.is_cuda or g.dtype != torch.float64 or tuple(g.shape) != (N,) or not g.is_contiguous():
        raise _lib.PesrHipError(f"gram_bwd.g: expected a contiguous float64 GPU tensor [{N}]")
    gf = torch.empty_like(f)
    rc = _lib.lib().pesr_gram_bwd(_p(f), _p(dg), _p(g), _p(gf), N, H, W, C, ph, pw, _stream())
    _lib.check(rc, "pesr_gram_bwd")
    return gf


# ------------------------------------------------------------------------------------------------
# contextual loss (docs/modes.md section 4r): the stages of pesr_amd/csrc/cx.hip, separately callable
# ------------------------------------------------------------------------------------------------
CX_MAX_POINTS = 4096


def _chk_cx(what: str, t, shape, dtype=torch.float32):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        want = "" if shape is None else f" {list(shape)}"
        raise _lib.PesrHipError(f"{what}: expected a contiguous {str(dtype).replace('torch.', '')} GPU tensor{want} (there is no CPU path)")


def _chk_cx_shape(what: str, N: int, P: int, C: int):
    if C not in GRAM_CHANNELS:
        raise _lib.PesrHipError(f"{what}: C = {C}, the contextual kernels take C in {GRAM_CHANNELS}")
    if not 1 <= P <= CX_MAX_POINTS:
        raise _lib.PesrHipError(f"{what}: P = {P} points per image, the contextual kernels take 1 .. {CX_MAX_POINTS}")
    if not 1 <= N <= 65535:
        raise _lib.PesrHipError(f"{what}: N = {N}, the contextual kernels take 1 .. 65535 images")


def cx_plan(N: int, P: int, C: int) -> dict:
    """What the contextual kernels do with N images of P points and C channels (a host-only question): {"row_blocks": the blocks of 64
    rows of the distance and the row kernels; "col_pieces": the pieces of 64 columns the distance kernel stages; "workspace_bytes": what
    cx_fwd and cx_bwd want; "saved_bytes": what a forward keeps for its backward}.  ValueError for a shape the kernels do not take."""
    rb = _memo("pesr_cx_row_blocks", N, P, C)
    if rb < 1:
        raise ValueError(f"cx_plan: no contextual kernel for N {N}, P {P}, C {C}")
    return {"row_blocks": rb, "col_pieces": _memo("pesr_cx_col_pieces", N, P, C),
            "workspace_bytes": int(_lib.lib().pesr_cx_workspace_bytes(N, P, C)), "saved_bytes": int(_lib.lib().pesr_cx_saved_bytes(N, P, C))}


def cx_normalize(fa: torch.Tensor, fb: torch.Tensor):
    """NHWC features fa (sr), fb (hr) [N, H, W, C] -> (xh, yh, inv, mu): both centred on fb's mean mu [N, C] and scaled to unit length
    (smooth at 0), fp32 [N, P, C] with P = H W row-major; inv [N, P] = 1 / sqrt(|fa - mu|^2 + 1e-12), what the backward needs."""
    for name, f in (("fa", fa), ("fb", fb)):
        if not torch.is_tensor(f) or not f.is_cuda or f.dtype != torch.float32 or f.dim() != 4 or not f.is_contiguous():
            raise _lib.PesrHipError(f"cx_normalize.{name}: expected contiguous [N, H, W, C] float32 GPU tensors (NHWC features; there is no "
                                    "CPU path)")
    if tuple(fa.shape) != tuple(fb.shape):
        raise _lib.PesrHipError(f"cx_normalize: the two tensors differ in shape: {tuple(fa.shape)} and {tuple(fb.shape)}")
    N, H, W, C = fa.shape
    P = H * W
    _chk_cx_shape("cx_normalize", N, P, C)
    xh = torch.empty((N, P, C), dtype=torch.float32, device=fa.device)
    yh, inv, mu = torch.empty_like(xh), xh.new_empty((N, P)), xh.new_empty((N, C))
    rc = _lib.lib().pesr_cx_normalize(_p(fa), _p(fb), _p(mu), _p(xh), _p(yh), _p(inv), N, P, C, _stream())
    _lib.check(rc, "pesr_cx_normalize")
    return xh, yh, inv, mu


def cx_dist(xh: torch.Tensor, yh: torch.Tensor):
    """(xh, yh) fp32 [N, P, C] -> (D fp32 [N, P, P] = (1 - xh_i . yh_j) / 2 on the fp32 MFMA, m fp32 [N, P] = min_k D_ik, b int32 [N, P] its
    lowest index)."""
    _chk_cx("cx_dist.xh", xh, None)
    if xh.dim() != 3:
        raise _lib.PesrHipError(f"cx_dist.xh: expected [N, P, C], got {tuple(xh.shape)}")
    _chk_cx("cx_dist.yh", yh, xh.shape)
    N, P, C = xh.shape
    _chk_cx_shape("cx_dist", N, P, C)
    D = torch.empty((N, P, P), dtype=torch.float32, device=xh.device)
    m = torch.empty((N, P), dtype=torch.float32, device=xh.device)
    b = torch.empty((N, P), dtype=torch.int32, device=xh.device)
    rc = _lib.lib().pesr_cx_dist(_p(xh), _p(yh), _p(D), _p(m), _p(b), N, P, C, _stream())
    _lib.check(rc, "pesr_cx_dist")
    return D, m, b


def cx_fwd(D: torch.Tensor, m: torch.Tensor, h: float = 0.5, C: int = 256):
    """(D, m) of cx_dist -> (L float64 [N] = -log CX, CX float64 [N], S fp32 [N, P] the row sums of the weights, a int32 [N, P] the arg
    max over i of c_ij (lowest i), cmax fp32 [N, P] that maximum).  h > 0 is the bandwidth; C only names the plan."""
    _chk_cx("cx_fwd.D", D, None)
    if D.dim() != 3 or D.shape[1] != D.shape[2]:
        raise _lib.PesrHipError(f"cx_fwd.D: expected [N, P, P], got {tuple(D.shape)}")
    N, P = D.shape[0], D.shape[1]
    _chk_cx("cx_fwd.m", m, (N, P))
    _chk_cx_shape("cx_fwd", N, P, C)
    if not float(h) > 0:
        raise _lib.PesrHipError(f"cx_fwd: h must be > 0, got {h}")
    S, cmax = torch.empty_like(m), torch.empty_like(m)
    a = torch.empty((N, P), dtype=torch.int32, device=D.device)
    CX = torch.empty(N, dtype=torch.float64, device=D.device)
    L = torch.empty_like(CX)
    ws = workspace(cx_plan(N, P, C)["workspace_bytes"], D.device)
    rc = _lib.lib().pesr_cx_fwd(_p(D), _p(m), float(h), _p(S), _p(a), _p(cmax), _p(CX), _p(L), N, P, C, _p(ws), ws.numel(), _stream())
    _lib.check(rc, "pesr_cx_fwd")
    return L, CX, S, a, cmax


def cx_bwd(gL: torch.Tensor, xh, yh, inv, D, m, b, S, a, cmax, CX, h: float = 0.5, shape=None, parts: bool = False):
    """The gradient of sum_n gL[n] L[n] with respect to the sr features, the selections a, b held fixed: fp32 [N, H, W, C] (`shape`;
    default [N, P, 1, C]).  gL: device double [N]; the rest is what cx_normalize, cx_dist and cx_fwd returned.  Not masked by fa > 0.
    parts=True: -> (gf, E fp32 [N, P, P] = dL/dD, g_xh fp32 [N, P, C] = -E yh / 2), the two intermediates, for tests."""
    _chk_cx("cx_bwd.xh", xh, None)
    if xh.dim() != 3:
        raise _lib.PesrHipError(f"cx_bwd.xh: expected [N, P, C], got {tuple(xh.shape)}")
    N, P, C = xh.shape
    _chk_cx_shape("cx_bwd", N, P, C)
    _chk_cx("cx_bwd.yh", yh, (N, P, C))
    _chk_cx("cx_bwd.D", D, (N, P, P))
    for name, t in (("inv", inv), ("m", m), ("S", S), ("cmax", cmax)):
        _chk_cx("cx_bwd." + name, t, (N, P))
    for name, t in (("a", a), ("b", b)):
        _chk_cx("cx_bwd." + name, t, (N, P), torch.int32)
    for name, t in (("gL", gL), ("CX", CX)):
        _chk_cx("cx_bwd." + name, t, (N,), torch.float64)
    if not float(h) > 0:
        raise _lib.PesrHipError(f"cx_bwd: h must be > 0, got {h}")
    shape = (N, P, 1, C) if shape is None else tuple(shape)
    if len(shape) != 4 or shape[0] != N or shape[1] * shape[2] != P or shape[3] != C:
        raise _lib.PesrHipError(f"cx_bwd: shape {shape} is not [N, H, W, C] of {N} x {P} points x {C}")
    gf = torch.empty(shape, dtype=torch.float32, device=xh.device)
    E = torch.empty_like(D) if parts else None
    gxh = torch.empty_like(xh) if parts else None
    ws = workspace(cx_plan(N, P, C)["workspace_bytes"], xh.device)
    rc = _lib.lib().pesr_cx_bwd(_p(D), _p(m), _p(b), _p(S), _p(a), _p(cmax), _p(CX), _p(gL), _p(xh), _p(yh), _p(inv), float(h), _p(gf),
                                _p(E), _p(gxh), N, P, C, _p(ws), ws.numel(), _stream())
    _lib.check(rc, "pesr_cx_bwd")
    return (gf, E, gxh) if parts else gf


# ------------------------------------------------------------------------------------------------
# tiled inference (docs/modes.md section 4h; the plan and the driver are pesr_amd/tile.py)
# ------------------------------------------------------------------------------------------------
def _tile_desc(desc, cols: int, device):
    """Descriptor rows as a C-contiguous int32 host array (what the library checks) and its copy on the device (what the kernel
    reads)."""
    import numpy as np
    host = np.ascontiguousarray(np.asarray(desc, dtype=np.int32).reshape(-1, cols))
    return host, torch.from_numpy(host).to(device)


def _entry_layout(t: torch.Tensor, name: str):
    """_image_layout of a tile_scatter argument (the Generator's outputs and their slices are in one of the two: never the copy)."""
    return _image_layout(t, f"tile_scatter: {name}: expected an [n, 3, h, w] float32 GPU tensor")


def tile_gather(src: torch.Tensor, desc, oh: int, ow: int) -> torch.Tensor:
    """Tiles of one LR image as a batch.  src: fp32 [3, H, W] or uint8 [H, W, 3] device tensor; desc: rows {y0, x0, member};
    -> fp32 [n, 3, oh, ow], entry i = member desc[i][2] (entry of test.py:x8_forward's inputs) of the tile at (y0, x0)."""
    if not (torch.is_tensor(src) and src.is_cuda):
        raise _lib.PesrHipError("tile_gather needs a device tensor: pesr_amd has no CPU fallback")
    if src.dtype == torch.uint8 and src.dim() == 3 and src.shape[2] == 3:
        u8, H, W = 1, int(src.shape[0]), int(src.shape[1])
    elif src.dtype == torch.float32 and src.dim() == 3 and src.shape[0] == 3:
        u8, H, W = 0, int(src.shape[1]), int(src.shape[2])
    else:
        raise _lib.PesrHipError("tile_gather: expected a float32 [3, H, W] or a uint8 [H, W, 3] image")
    src = src.contiguous()
    host, dev = _tile_desc(desc, 3, src.device)
    n = host.shape[0]
    out = torch.empty((n, 3, int(oh), int(ow)), dtype=torch.float32, device=src.device)
    rc = _lib.lib().pesr_tile_gather(src.data_ptr(), u8, H, W, out.data_ptr(), host.ctypes.data, dev.data_ptr(), n, int(oh), int(ow),
                                     _stream())
    _lib.check(rc, "pesr_tile_gather")
    return out


def tile_scatter(t_lo: torch.Tensor, t_hi: Optional[torch.Tensor], desc, E: int, th: int, tw: int, s: int, H: int, W: int,
                 out_f32: Optional[torch.Tensor] = None, out_u8: Optional[torch.Tensor] = None, p: Optional[torch.Tensor] = None,
                 wa: float = 1.0, wb: float = 0.0) -> None:
    """The owned pixels of n / E tiles into the fp32 [3, s*H, s*W] and / or uint8 [s*H, s*W, 3] image.  t_lo: the Generator's outputs
    [n, 3, s*th, s*tw] (with t_hi: members 0-3 there, members 4-7 [n, 3, s*tw, s*th] in t_hi); desc: rows {y0, x0, oy, ox, oh, ow};
    p: the E = 1 outputs of a second model for the blend wa * p + wb * v (wa, wb are rounded to fp32 here)."""
    import numpy as np
    t_lo, lay = _entry_layout(t_lo, "t_lo")
    n = int(t_lo.shape[0])
    if t_hi is not None:
        t_hi, lay_hi = _entry_layout(t_hi, "t_hi")
        if lay_hi != lay:
            t_lo, t_hi, lay = t_lo.contiguous(), t_hi.contiguous(), 0
        if tuple(t_hi.shape) != (n, 3, s * tw, s * th):
            raise ValueError(f"tile_scatter: t_hi is {tuple(t_hi.shape)}, expected {(n, 3, s * tw, s * th)}")
        n *= 2
    if tuple(t_lo.shape[1:]) != (3, s * th, s * tw):
        raise ValueError(f"tile_scatter: t_lo is {tuple(t_lo.shape)}, expected [n, 3, {s * th}, {s * tw}]")
    lay_p = 0
    if p is not None:
        p, lay_p = _entry_layout(p, "p")
        if tuple(p.shape) != (n // max(int(E), 1), 3, s * th, s * tw):
            raise ValueError(f"tile_scatter: p is {tuple(p.shape)}, expected {(n // max(int(E), 1), 3, s * th, s * tw)}")
    if out_f32 is not None:
        if not (out_f32.is_cuda and out_f32.dtype == torch.float32 and out_f32.is_contiguous() and tuple(out_f32.shape) == (3, s * H, s * W)):
            raise ValueError(f"tile_scatter: out_f32 must be a contiguous float32 GPU tensor [3, {s * H}, {s * W}]")
    if out_u8 is not None:
        if not (out_u8.is_cuda and out_u8.dtype == torch.uint8 and out_u8.is_contiguous() and tuple(out_u8.shape) == (s * H, s * W, 3)):
            raise ValueError(f"tile_scatter: out_u8 must be a contiguous uint8 GPU tensor [{s * H}, {s * W}, 3]")
    host, dev = _tile_desc(desc, 6, t_lo.device)
    if host.shape[0] * int(E) != n:
        raise ValueError(f"tile_scatter: {host.shape[0]} descriptor rows for {n} entries with E = {E}")
    rc = _lib.lib().pesr_tile_scatter(t_lo.data_ptr(), None if t_hi is None else t_hi.data_ptr(), lay, None if p is None else p.data_ptr(),
                                      lay_p, float(np.float32(wa)), float(np.float32(wb)), host.ctypes.data, dev.data_ptr(), n, int(E),
                                      int(th), int(tw), int(s), int(H), int(W), None if out_f32 is None else out_f32.data_ptr(),
                                      None if out_u8 is None else out_u8.data_ptr(), _stream())
    _lib.check(rc, "pesr_tile_scatter")


# ------------------------------------------------------------------------------------------------
# spectral normalisation (reference model/basic.py:25; torch.nn.utils.spectral_norm semantics)
# ------------------------------------------------------------------------------------------------
def spectral_norm_fwd(w: torch.Tensor, u: torch.Tensor, v: torch.Tensor, update: bool, eps: float = 1e-12):
    """w [O, ...] -> (w_hat = w / sigma, sigma [1]); update: one power iteration first, u and v rewritten IN PLACE."""
    for t, n in ((w, "w"), (u, "u"), (v, "v")):
        _chk(t, "spectral_norm_fwd." + n)
    O = w.shape[0]
    K = w.numel() // O
    assert u.numel() == O and v.numel() == K
    L = _lib.lib()
    ws = workspace(L.pesr_spectral_norm_workspace_bytes(O, K), w.device)
    w_hat = torch.empty_like(w)
    sigma = torch.empty(1, dtype=torch.float32, device=w.device)
    rc = L.pesr_spectral_norm_fwd(_p(w), _p(u), _p(v), _p(w_hat), _p(sigma), O, K, int(update), eps, _p(ws), ws.numel(), _stream())
    _lib.check(rc, f"pesr_spectral_norm_fwd[{O}x{K}]")
    return w_hat, sigma


def spectral_norm_bwd(g: torch.Tensor, w_hat: torch.Tensor, u: torch.Tensor, v: torch.Tensor, sigma: torch.Tensor, dw_out=None,
                      accumulate: bool = False):
    """dL/dw for g = dL/d(w_hat) with the u, v, sigma of that forward."""
    _chk(g, "spectral_norm_bwd.g")
    O = g.shape[0]
    K = g.numel() // O
    L = _lib.lib()
    ws = workspace(L.pesr_spectral_norm_workspace_bytes(O, K), g.device)
    assert not accumulate or dw_out is not None
    dw = _out(dw_out, tuple(g.shape), g.device)
    rc = L.pesr_spectral_norm_bwd(_p(g), _p(w_hat), _p(u), _p(v), _p(sigma), _p(dw), O, K, int(accumulate), _p(ws), ws.numel(), _stream())
    _lib.check(rc, f"pesr_spectral_norm_bwd[{O}x{K}]")
    return dw


# ------------------------------------------------------------------------------------------------
# generic k x k conv (odd k != 3): compatibility path of reference model/basic.py:4-7
# ------------------------------------------------------------------------------------------------
def conv_kxk_fwd(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stride: int = 1) -> torch.Tensor:
    _chk(x, "conv_kxk_fwd.x"); _chk(w, "conv_kxk_fwd.w")
    N, H, W, Cin = x.shape
    Cout, k = w.shape[0], w.shape[2]
    assert w.shape == (Cout, Cin, k, k)
    y = torch.empty((N, (H - 1) // stride + 1, (W - 1) // stride + 1, Cout), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().pesr_conv_kxk_fwd(_p(x), _p(w), _p(bias), _p(y), N, H, W, Cin, Cout, k, stride, _stream()), f"pesr_conv_kxk_fwd[k={k}]")
    return y


def conv_kxk_dgrad(dy: torch.Tensor, w: torch.Tensor, in_shape, stride: int = 1) -> torch.Tensor:
    _chk(dy, "conv_kxk_dgrad.dy"); _chk(w, "conv_kxk_dgrad.w")
    N, H, W, Cin = in_shape
    Cout, k = w.shape[0], w.shape[2]
    dx = torch.empty((N, H, W, Cin), dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib().pesr_conv_kxk_dgrad(_p(dy), _p(w), _p(dx), N, H, W, Cin, Cout, k, stride, _stream()), f"pesr_conv_kxk_dgrad[k={k}]")
    return dx


def conv_kxk_wgrad(x: torch.Tensor, dy: torch.Tensor, k: int, stride: int = 1, want_bias: bool = True, dw_out=None, db_out=None):
    _chk(x, "conv_kxk_wgrad.x"); _chk(dy, "conv_kxk_wgrad.dy")
    N, H, W, Cin = x.shape
    Cout = dy.shape[3]
    dw = _out(dw_out, (Cout, Cin, k, k), x.device)
    db = _out(db_out, (Cout,), x.device) if want_bias else None
    _lib.check(_lib.lib().pesr_conv_kxk_wgrad(_p(x), _p(dy), _p(dw), _p(db), N, H, W, Cin, Cout, k, stride, _stream()), f"pesr_conv_kxk_wgrad[k={k}]")
    return dw, db


# ------------------------------------------------------------------------------------------------
# GAN losses on the logits (reference train.py:210-213,244-253; model/focal_loss.py)
# ------------------------------------------------------------------------------------------------
GAN_TYPES = {"SGAN": 0, "RSGAN": 1, "RaSGAN": 2}


def gan_loss(pred_real: torch.Tensor, pred_fake: torch.Tensor, gan_type: str, side: int, focal: bool, gamma: float, scale: float = 1.0,
             need_real: bool = True, need_fake: bool = True):
    """-> (out [1] = scale * loss, d_real [B,1] | None, d_fake [B,1] | None): value and gradients in one launch."""
    _chk(pred_real, "gan_loss.pred_real"); _chk(pred_fake, "gan_loss.pred_fake")
    B = pred_real.numel()
    assert pred_fake.numel() == B
    out = torch.empty(1, dtype=torch.float32, device=pred_real.device)
    d_r = torch.empty_like(pred_real) if need_real else None
    d_f = torch.empty_like(pred_fake) if need_fake else None
    rc = _lib.lib().pesr_gan_loss_fwd_bwd(_p(pred_real), _p(pred_fake), B, GAN_TYPES[gan_type], side, int(focal), float(gamma), float(scale),
                                          _p(out), _p(d_r), _p(d_f), _stream())
    _lib.check(rc, f"pesr_gan_loss_fwd_bwd[{gan_type}, side {side}]")
    return out, d_r, d_f


def gan_loss_map(pred_real: torch.Tensor, pred_fake: torch.Tensor, gan_type: str, side: int, focal: bool, gamma: float, scale: float = 1.0,
                 need_real: bool = True, need_fake: bool = True):
    """The same definitions on a logit map of any shape and size (docs/modes.md section 4v): -> (out [1] = scale * the mean over all
    elements, d_real | None, d_fake | None shaped like the logits).  RSGAN pairs the logits of one index, RaSGAN's means run over every
    element.  Two launches (RaSGAN: five), per-workgroup fp32 rows added in double in a fixed order."""
    _chk(pred_real, "gan_loss_map.pred_real"); _chk(pred_fake, "gan_loss_map.pred_fake")
    n = pred_real.numel()
    if n < 1:
        raise ValueError(f"gan_loss_map.pred_real: an empty tensor {tuple(pred_real.shape)}")
    if pred_fake.shape != pred_real.shape:
        raise ValueError(f"gan_loss_map.pred_fake: expected {tuple(pred_real.shape)}, got {tuple(pred_fake.shape)}")
    if gan_type not in GAN_TYPES:
        raise ValueError(f"gan_loss_map.gan_type: {gan_type!r}; one of {tuple(GAN_TYPES)}")
    if side not in (0, 1):
        raise ValueError(f"gan_loss_map.side: {side!r}; 0 (discriminator) or 1 (generator)")
    L = _lib.lib()
    out = torch.empty(1, dtype=torch.float32, device=pred_real.device)
    d_r = torch.empty_like(pred_real) if need_real else None
    d_f = torch.empty_like(pred_fake) if need_fake else None
    ws = workspace(int(L.pesr_gan_loss_map_workspace_bytes(n)), pred_real.device)
    rc = L.pesr_gan_loss_map(_p(pred_real), _p(pred_fake), n, GAN_TYPES[gan_type], side, int(focal), float(gamma), float(scale), _p(out),
                             _p(d_r), _p(d_f), _p(ws), ws.numel(), _stream())
    _lib.check(rc, f"pesr_gan_loss_map[{gan_type}, side {side}, n {n}]")
    return out, d_r, d_f
