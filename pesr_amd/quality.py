"""What a run scores and how it prints it, once for test.py and train.py's validation: PSNR-Y always, SSIM-Y (docs/modes.md section 4g),
NIQE (section 4k), LPIPS (section 4n) and DISTS (section 4t) when asked for, in that column order, through utils.compute_PSNR /
compute_SSIM / compute_NIQE / compute_LPIPS / compute_DISTS.  One --shave rule and one "the image must hold the model" pre-check serve both programs; what differs
between them (flag names, labels, digits, the tensorboard tag) is in the table below.
"""
import numpy as np

# column -> (test.py's value with its unit, train.py's name, train.py's value with its unit); the tensorboard tag is "Validate <name>"
_COLUMNS = {
    "PSNR-Y": ("%.10f dB", "PSNR", "%.4fdB"),
    "SSIM-Y": ("%.10f", "SSIM", "%.6f"),
    "NIQE": ("%.10f", "NIQE", "%.6f"),
    "LPIPS": ("%.10f", "LPIPS", "%.6f"),
    "DISTS": ("%.10f", "DISTS", "%.6f"),
}


class ScoreError(ValueError):
    """The ValueError of a score that takes a model (NIQE, LPIPS, DISTS) for an image it cannot take; `flags` names the model's flag and
    the shave's, for the entry point's own wording of the refusal."""

    def __init__(self, flags, err):
        super().__init__(str(err))
        self.flags = flags


class Scorer:
    def __init__(self, prog, ssim, shave, niqe="", lpips="", flags=("--niqe", "--lpips", "--shave"), size_flags=None, have_hr=True,
                 dists="", dists_flag="--dists"):
        """prog and flags (of the NIQE model, the LPIPS model and the shave; size_flags: all that decide an image's size after the
        shave, the shave's alone by default) and dists_flag (of the DISTS model) are quoted in the refusals.  niqe / lpips / dists: a model
        file (or a loaded model), "" = that column is off.  have_hr false: a run without HR images, which LPIPS and DISTS refuse.  SystemExit naming the flag for a file that is no
        model.  No GPU is touched."""
        self.prog, self.ssim, self.shave = prog, bool(ssim), int(shave)
        self.niqe_flag, self.lpips_flag, self.shave_flag = flags
        self.size_flags = size_flags or self.shave_flag
        self.dists_flag = dists_flag
        self.niqe_model = self.lpips_model = self.dists_model = None
        if niqe:
            from . import niqe as _niqe
            self.niqe_model = _niqe.load_model_flag(prog, self.niqe_flag, niqe) if isinstance(niqe, str) else niqe
        if lpips:
            if not have_hr:
                raise SystemExit(f"{prog}: {self.lpips_flag} compares the result with the HR image: it needs --from_hr true")
            from . import lpips as _lpips
            self.lpips_model = _lpips.load_model_flag(prog, self.lpips_flag, lpips) if isinstance(lpips, str) else lpips

        if dists:
            if not have_hr:
                raise SystemExit(f"{prog}: {self.dists_flag} compares the result with the HR image: it needs --from_hr true")
            from . import dists as _dists
            self.dists_model = _dists.load_model_flag(prog, self.dists_flag, dists) if isinstance(dists, str) else dists

    def columns(self, hr=True):
        """The names of the values score() returns, in its order; without an HR image only NIQE can be measured."""
        on = {"PSNR-Y": hr, "SSIM-Y": hr and self.ssim, "NIQE": self.niqe_model is not None, "LPIPS": hr and self.lpips_model is not None,
              "DISTS": hr and self.dists_model is not None}
        return [c for c in _COLUMNS if on[c]]

    def check_size(self, h, w, name):
        """SystemExit unless an h x w image (`name` in the message) holds, after the shave, the NIQE model's block twice and LPIPS's
        and DISTS's 16 x 16.  Only the size is needed - a PNG header's, or the synthetic patch's: no GPU is touched."""
        if self.niqe_model is not None:
            from . import niqe as _niqe
            _niqe.check_fits_flag(self.prog, f"{self.niqe_flag} / {self.size_flags}", self.niqe_model, h, w, self.shave, name)
        if self.lpips_model is not None:
            from .lpips import MIN_SIDE
            if min(h, w) - 2 * self.shave < MIN_SIDE:
                raise SystemExit(f"{self.prog}: {self.lpips_flag} / {self.size_flags}: {name}: {max(h - 2 * self.shave, 0)} x "
                                 f"{max(w - 2 * self.shave, 0)} after the shave; LPIPS needs at least {MIN_SIDE} x {MIN_SIDE}")
        if self.dists_model is not None:
            from .lpips import MIN_SIDE
            if min(h, w) - 2 * self.shave < MIN_SIDE:
                raise SystemExit(f"{self.prog}: {self.dists_flag} / {self.size_flags}: {name}: {max(h - 2 * self.shave, 0)} x "
                                 f"{max(w - 2 * self.shave, 0)} after the shave; DISTS needs at least {MIN_SIDE} x {MIN_SIDE}")

    def score(self, sr, hr=None):
        """[1,3,H,W] result (and HR image) -> {column: value} in columns(hr is not None)'s order.  LPIPS and DISTS are taken of the uint8
        values the result would be saved as (the identity on an image read back from its file)."""
        import utils
        out = {}
        for c in self.columns(hr is not None):
            try:
                if c == "PSNR-Y":
                    out[c] = utils.compute_PSNR(sr, hr, self.shave)
                elif c == "SSIM-Y":
                    out[c] = utils.compute_SSIM(sr, hr, self.shave)
                elif c == "NIQE":
                    out[c] = utils.compute_NIQE(sr, self.niqe_model, self.shave)
                elif c == "LPIPS":
                    out[c] = utils.compute_LPIPS(sr.clamp(0, 255).round(), hr, self.lpips_model, self.shave)
                else:
                    out[c] = utils.compute_DISTS(sr.clamp(0, 255).round(), hr, self.dists_model, self.shave)
            except ValueError as e:
                flag = {"NIQE": self.niqe_flag, "LPIPS": self.lpips_flag, "DISTS": self.dists_flag}.get(c)
                if flag:
                    raise ScoreError(f"{flag} / {self.shave_flag}", e) from None
                raise
        return out

    @staticmethod
    def mean(rows, columns=()):
        """The column means of score()'s results (0.0 for each of `columns` when there are none)."""
        return {c: float(np.mean([r[c] for r in rows])) if rows else 0.0 for c in (rows[0] if rows else columns)}

    @staticmethod
    def test_line(values, bicubic=None):
        """test.py: "PSNR-Y V dB, bicubic B dB, SSIM-Y V, bicubic B, ..." of a result's values and the bicubic baseline's, or
        "NIQE V" alone without a baseline; after "<file>: " for an image, after "Mean " for the set."""
        return ", ".join(c + " " + _COLUMNS[c][0] % v + (", bicubic " + _COLUMNS[c][0] % bicubic[c] if bicubic else "") for c, v in values.items())

    @staticmethod
    def valid_lines(epoch, epochs, means, psnr_tag=""):
        """train.py: per column (the line "Finish valid [e/E]. NAME: V", the tensorboard tag, the value)."""
        for c, v in means.items():
            _, name, fmt = _COLUMNS[c]
            yield ("Finish valid [%d/%d]. %s: " % (epoch, epochs, name) + fmt % v + (psnr_tag if c == "PSNR-Y" else ""), "Validate " + name, v)
