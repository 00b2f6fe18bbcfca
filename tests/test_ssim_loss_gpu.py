"""GPU: SSIM-Y as a training loss (docs/modes.md section 4p).

Score, coefficient maps and gradient of pesr_amd/csrc/ssim.hip's loss kernels against tests/ssim_loss_oracle.py BIT FOR BIT: the kernels' order
of operations is fixed and nothing is fused, so kernel and restatement perform the same IEEE operations, the score's summation tree and
the gradient's one rounding to float32 included.  How far the ordered gradient is from autograd on the definition is bounded on the CPU
(tests/test_ssim_loss_cpu.py).  Then the layouts, the margins, and the training steps with the term off, on and captured."""
import numpy as np
import pytest
import torch

import ssim_loss_cases as C
import ssim_loss_oracle as O
import loss_step_harness as HS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
LAYOUTS = [(False, True), (True, False), (False, False), (True, True)]        # (a channels_last, b channels_last)


def _dev(x, channels_last=False):
    t = torch.from_numpy(np.array(x)).to(DEV)
    return t.contiguous(memory_format=torch.channels_last) if channels_last else t


def _same_bits(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    kind = np.int32 if got.dtype == np.float32 else np.int64
    gb, wb = np.ascontiguousarray(got).view(kind), np.ascontiguousarray(want).view(kind)
    if not np.array_equal(gb, wb):
        bad = np.argwhere(gb != wb)
        pytest.fail(f"{what}: {len(bad)} of {want.size} elements differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]!r} != "
                    f"{want[tuple(bad[0])]!r}, max |diff| {np.max(np.abs(got.astype(np.float64) - want)):.3e}")


def _check(kind, n, h, w, a_cl, b_cl):
    from pesr_amd import ops
    a, b, g = C.case(kind, n, h, w)
    score_w, coef_w, grad_w = C.ordered(kind, n, h, w)
    what = f"{kind} {n} x {h} x {w} a {'NHWC' if a_cl else 'NCHW'} b {'NHWC' if b_cl else 'NCHW'}"
    da, db, dg = _dev(a, a_cl), _dev(b, b_cl), _dev(g)
    score, coef = ops.ssim_loss_fwd(da, db, True)
    assert score.dtype == torch.float64 and score.shape == (n,) and coef.shape == (n, 3, h - 10, w - 10) and coef.is_contiguous()
    _same_bits(score, score_w, what + ": score")
    _same_bits(coef, coef_w, what + ": coef")
    plain, none = ops.ssim_loss_fwd(da, db, False)
    assert none is None and torch.equal(plain, score)                 # the pure score: the same bits, no coefficients
    ga = ops.ssim_loss_bwd(da, db, coef, dg)
    assert ga.dtype == torch.float32 and ga.shape == da.shape and ga.stride() == da.stride()
    _same_bits(ga, grad_w, what + ": gradient")
    assert torch.equal(ops.ssim_loss_bwd(da, db, coef, dg), ga)       # the same bits on every call
    return score_w, grad_w


# ---- the kernels, bit for bit -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", C.SHAPES)
def test_score_coefficients_and_gradient_bit_for_bit(h, w):
    """sr = integer hr + noise reaching below 0 and above 255 (nothing clips), every layout pair, N = 1 and 3 with a different g per
    image."""
    for n in C.BATCHES:
        a, _, g = C.case("noise", n, h, w)
        assert a.min() < 0 and a.max() > 255 and len(set(g.tolist())) == n
        for a_cl, b_cl in LAYOUTS:
            score, grad = _check("noise", n, h, w, a_cl, b_cl)
        assert np.isfinite(grad).all() and np.abs(grad).max() > 0 and bool((score < 1).all())


@pytest.mark.parametrize("h,w", C.SHAPES)
def test_special_inputs_bit_for_bit(h, w):
    """a == b (score exactly 1.0), two constant images that differ by 3, a constant image against noise."""
    for i, kind in enumerate(("same", "const", "const_noise")):
        for n in C.BATCHES:
            score, grad = _check(kind, n, h, w, *LAYOUTS[(i + n) % 4])
            assert np.isfinite(grad).all()
            if kind == "same":
                assert score.tolist() == [1.0] * n


def test_score_of_more_partials_than_lanes_bit_for_bit():
    """267 x 491: a 257 x 481 map, 17 x 16 = 272 tiles per image, so the mean of an image's partials (reduce.hip, shared with the SSIM-Y
    score, the LPIPS head and the Gram distance) takes a second round of its lane loop, a tail of 16.  No smaller shape above does."""
    from pesr_amd import ops
    n, h, w = 2, 267, 491
    assert -(-(h - 10) // O.TILE_H) * -(-(w - 10) // O.TILE_W) == O.LANES + 16
    a, b, _ = C.case("noise", n, h, w)
    score, _ = ops.ssim_loss_fwd(_dev(a), _dev(b))
    _same_bits(score, O.score_ordered(a, b), f"noise {n} x {h} x {w}: score")


def test_margins_come_back_intact():
    """Through the C ABI: the inputs sit between NaNs (a read outside would poison the result), every output between sentinels."""
    from pesr_amd import _lib
    lib = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    M, sentinel, n = 2048, -12345.678, 3

    def framed(arr, fill):
        t = torch.full((arr.size + 2 * M,), fill, dtype=torch.float32 if arr.dtype == np.float32 else torch.float64, device=DEV)
        t[M:M + arr.size] = _dev(arr).reshape(-1)
        return t

    def intact(t, size, fill):
        return bool((t[:M] == fill).all()) and bool((t[M + size:] == fill).all())

    for (h, w), nhwc in (((13, 15), 0), ((27, 43), 1), ((47, 80), 0), ((47, 80), 1)):
        a, b, g = C.case("noise", n, h, w)
        score_w, coef_w, grad_w = C.ordered("noise", n, h, w)
        lay = (lambda x: np.ascontiguousarray(x.transpose(0, 2, 3, 1))) if nhwc else (lambda x: x)
        fa, fb, fg = framed(lay(a), float("nan")), framed(lay(b), float("nan")), framed(g, float("nan"))
        score, coef = framed(np.zeros(n), sentinel), framed(np.zeros(coef_w.shape), sentinel)
        ga = framed(np.zeros(a.shape, np.float32), sentinel)
        ws = torch.full((n * 9 + 2 * M,), sentinel, dtype=torch.float64, device=DEV)
        ptr = lambda t: t.data_ptr() + t.element_size() * M
        assert lib.pesr_ssim_loss_fwd(ptr(fa), ptr(fb), ptr(score), n, h, w, nhwc, nhwc, ptr(coef), ptr(ws), 8 * n * 9, stream) == 0
        assert lib.pesr_ssim_loss_bwd(ptr(fa), ptr(fb), ptr(coef), ptr(fg), ptr(ga), n, h, w, nhwc, nhwc, stream) == 0
        torch.cuda.synchronize()
        assert intact(score, n, sentinel) and intact(coef, coef_w.size, sentinel) and intact(ws, n * 9, sentinel)
        assert intact(ga, a.size, np.float32(sentinel))
        _same_bits(score[M:M + n], score_w, "score")
        _same_bits(coef[M:M + coef_w.size].reshape(coef_w.shape), coef_w, "coef")
        _same_bits(ga[M:M + a.size].reshape(lay(a).shape), lay(grad_w), "gradient")
        # a refused call writes nothing
        keep = ga.clone()
        assert lib.pesr_ssim_loss_bwd(ptr(fa), ptr(fb), ptr(coef), ptr(fg) + 4, ptr(ga), n, h, w, nhwc, nhwc, stream) == -1
        assert lib.pesr_ssim_loss_fwd(ptr(fa), ptr(fb), ptr(score), n, h, w, nhwc, nhwc, ptr(coef), ptr(ws), 8, stream) == -2
        torch.cuda.synchronize()
        assert torch.equal(ga, keep) and intact(ws, n * 9, sentinel)


def test_function_gives_a_gradient_to_sr_only_in_its_layout():
    from pesr_amd import functional as PF
    n, h, w = 3, 27, 42
    a, b, g = C.case("noise", n, h, w)
    score_w, _, grad_w = C.ordered("noise", n, h, w)
    for a_cl in (False, True):
        sr, hr = _dev(a, a_cl).requires_grad_(), _dev(b, not a_cl).requires_grad_()
        score = PF.ssim_loss(sr, hr)
        assert score.dtype == torch.float64 and score.shape == (n,) and score.requires_grad
        (score * _dev(g)).sum().backward()
        assert hr.grad is None and sr.grad.stride() == sr.stride()
        _same_bits(sr.grad, grad_w, "autograd")
        _same_bits(score.detach(), score_w, "score")
    plain = PF.ssim_loss(_dev(a), _dev(b))                             # nothing needs a gradient: the pure score
    assert not plain.requires_grad
    _same_bits(plain, score_w, "score without a graph")
    from pesr_amd import _lib, ops
    with pytest.raises(ValueError, match="differ in shape"):
        ops.ssim_loss_fwd(_dev(a), _dev(b)[:, :, :, :30])
    with pytest.raises(ValueError, match="11 x 11"):
        ops.ssim_loss_fwd(_dev(a)[:, :, :10].contiguous(), _dev(b)[:, :, :10].contiguous())
    with pytest.raises(_lib.PesrHipError, match="coef"):
        ops.ssim_loss_bwd(_dev(a), _dev(b), torch.zeros(n, 3, h - 10, w - 9, dtype=torch.float64, device=DEV), _dev(g))
    with pytest.raises(_lib.PesrHipError, match="float64"):
        ops.ssim_loss_bwd(_dev(a), _dev(b), torch.zeros(n, 3, h - 10, w - 10, dtype=torch.float64, device=DEV), _dev(g).float())


# ---- the training steps -----------------------------------------------------------------------------------------------------------------
# (off, on beside the other logs, and captured: tests/test_loss_terms_gpu.py, for every term, on this harness)
BATCH, ALPHA = 4, 0.5                                                 # the toy networks of tests/test_lpips_loss_gpu.py; the HR side is 32
H = HS.harness(250, BATCH)                                            # 64 channels, 2 blocks, LR 8 x 8, lr 5e-5


@pytest.mark.parametrize("phase", ["pretrain", "train"])
def test_step_with_the_term_on(phase):
    lr, hr = H.data()[0]
    tr = H.trainer(phase, alpha_ssim=ALPHA)
    with torch.no_grad():
        sr0 = tr.G(lr)                                                # the sr of the first step: G before its update
    mean = float(np.mean(O.score_ordered(sr0.cpu().numpy(), hr.cpu().numpy())))
    want = float(np.float32(np.float32(1.0 - mean) * np.float32(ALPHA)))
    logs4, states4, _ = H.run(4, phase, alpha_ssim=ALPHA)
    got = logs4[0]["ssim"]
    print(f"{phase}: logged ssim term {got!r}, restated {want!r}")
    # to fp32: torch's mean of the four float64 scores may order its sum otherwise, which moves the float32 by one unit at most
    assert np.isfinite(got) and 0 < got < ALPHA and abs(got - want) <= 2.0 ** -23 * want
    logs0, states0, _ = H.run(2, phase)
    HS.assert_only_G_moved(logs4[0], states4[0], logs0[0], states0[0])
