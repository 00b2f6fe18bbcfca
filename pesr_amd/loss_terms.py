"""The optional terms of the generator's loss, one record each (docs/modes.md section 4s).

TERMS is the table: Trainer (pesr_amd/step.py) builds its terms from it, evaluates the ones that are on, adds them to the loss and logs
them; train.py's loss_terms_of checks the flags against it and names the epoch line's columns and the tensorboard tags from it.  The
mathematics lives where it did - lpips.py, functional.py, texture.py, contextual.py; a record only says what the call sites need to know:

    key      the key in a step's logs and in the epoch line
    title    the tensorboard tag
    flag     the weight's flag; its name without the dashes (`weight`) is also Trainer's keyword argument
    params   the term's other keyword arguments of Trainer (and flags of the same names) -> their defaults
    phases   the train phases whose step has the term
    taps     the vgg19.features indices it reads from the VGG pass of gan_step
    on       weight > 0 (and whatever else the term needs)
    check(side, what)          None, or why the term cannot take HR patches of side x side; touches no device
    value(sr, hr, taps_sr, taps_hr)   device float64 [B]; taps_*: the term's own taps, in the order of `taps`
    loss(...)                  the fp32 scalar that joins the sum: weight * the batch mean of value()

A new term is a class here, an entry of TERMS and its flags in train.py's parser.  A ValueError of a constructor begins with the name of
the keyword argument it refuses, which is the flag's name too: train.py puts the dashes in front.
"""
from __future__ import annotations

import os

from . import contextual, lpips, texture
from . import functional as PF


class Term:
    key = title = flag = None
    params = {}
    phases = ("train",)
    taps = ()
    needs_phase = "the term is no part of the generator's loss in"  # how wrong_phase's sentence goes on, up to the refused phase

    def __init_subclass__(cls):
        cls.flag, cls.weight = "--alpha_" + cls.key, "alpha_" + cls.key

    def __init__(self, **kw):
        alpha = kw.pop(self.weight, 0.0)
        self.alpha = float(alpha)
        if not self.alpha >= 0:                                     # (NaN too)
            raise ValueError(f"{self.weight} {alpha} must be >= 0 (0 = off)")
        for name, default in self.params.items():
            setattr(self, name, kw.pop(name, default))
        if kw:
            raise TypeError(f"{type(self).__name__}: unexpected keyword arguments {sorted(kw)}")
        self.on = self.alpha > 0

    @classmethod
    def from_flags(cls, args, prog, valid_lpips_model=None):
        """The parsed flags -> the term's keyword arguments; SystemExit naming `prog` and the flags."""
        return {name: getattr(args, name) for name in (cls.weight, *cls.params)}

    def wrong_phase(self, phase):
        """The refusal of a train phase that is not among `phases`."""
        return f"{self.flag} {self.alpha} needs --phase {' or '.join(self.phases)}: {self.needs_phase} --phase {phase}"

    def check(self, side, what=None):
        return None

    def value(self, sr, hr, taps_sr, taps_hr):
        raise NotImplementedError

    def loss(self, sr, hr, taps_sr, taps_hr):
        """A batch mean like l1 and vgg, so no world_size factor (float64 [B] -> fp32 scalar)."""
        return self.value(sr, hr, taps_sr, taps_hr).mean().float() * self.alpha


class Lpips(Term):
    """LPIPS of sr against hr (docs/modes.md section 4o): on only with a model AND a positive weight."""
    key, title = "lpips", "LPIPS Loss"
    params = {"lpips_model": None}

    def __init__(self, **kw):
        super().__init__(**kw)
        self.on = self.on and self.lpips_model is not None

    @classmethod
    def from_flags(cls, args, prog, valid_lpips_model=None):
        """--lpips_loss is loaded even with the weight 0 (a file that does not load is refused either way); when it names the file of
        --valid_lpips, whose model the caller passes, the object is shared.  Off, the model is None."""
        model = None
        if args.lpips_loss:
            if valid_lpips_model is not None and os.path.realpath(args.lpips_loss) == os.path.realpath(args.valid_lpips):
                model = valid_lpips_model
            else:
                model = lpips.load_model_flag(prog, "--lpips_loss", args.lpips_loss)
        if args.alpha_lpips > 0 and model is None:
            raise SystemExit(f"{prog}: --alpha_lpips {args.alpha_lpips} needs --lpips_loss WEIGHTS (an LPIPS weight file; the project ships "
                             "none)")
        return {"alpha_lpips": args.alpha_lpips, "lpips_model": model if args.alpha_lpips > 0 else None}

    def wrong_phase(self, phase):
        return (f"--alpha_lpips {self.alpha} / --lpips_loss: the LPIPS term belongs to the generator's loss of --phase train, not --phase "
                f"{phase}")

    def check(self, side, what=None):
        why = lpips.check_loss_side(side, side)
        return why and f"--alpha_lpips / --lpips_loss: {what or side}: {why}"

    def value(self, sr, hr, taps_sr, taps_hr):
        return lpips.lpips_loss(sr, hr, self.lpips_model)


class Ssim(Term):
    """1 - SSIM-Y (docs/modes.md section 4p), in both phases.  value() is the score; loss() is weight * (1 - its batch mean)."""
    key, title = "ssim", "SSIM Loss"
    phases = ("pretrain", "train")
    WINDOW = 11

    def check(self, side, what=None):
        if side < self.WINDOW:
            return f"--alpha_ssim {self.alpha}: {what or side} is smaller than the {self.WINDOW} x {self.WINDOW} window of the SSIM"
        return None

    def value(self, sr, hr, taps_sr, taps_hr):
        return PF.ssim_loss(sr, hr)

    def loss(self, sr, hr, taps_sr, taps_hr):
        return (1 - self.value(sr, hr, taps_sr, taps_hr).mean()).float() * self.alpha


class Texture(Term):
    """The distance of patch-wise Gram matrices of three VGG19 taps (docs/modes.md section 4q).  texture_patch: the side of the patches
    in each tap's own pixels, 0 = the whole map."""
    key, title = "texture", "Texture Loss"
    params = {"texture_patch": 16}
    taps = texture.TAPS                                             # VGG.TAPS: relu1_1, relu2_1, relu3_1
    needs_phase = "the texture loss reads taps of the VGG19 trunk, and no VGG runs in"

    def __init__(self, **kw):
        super().__init__(**kw)
        self.texture_patch = int(self.texture_patch)
        if self.texture_patch < 0:
            raise ValueError(f"texture_patch {self.texture_patch} must be >= 0 (0 = the whole map)")

    def check(self, side, what=None):
        why = texture.check_patch(side, side, self.texture_patch)
        return why and (f"--alpha_texture {self.alpha}: --texture_patch {self.texture_patch} with {what or side}: {why}; --texture_patch 0 "
                        "takes the whole map of every tap")

    def value(self, sr, hr, taps_sr, taps_hr):
        return texture.texture_from_taps(taps_sr, taps_hr, self.texture_patch)


class Contextual(Term):
    """-log CX of the VGG19 tap relu3_4 (docs/modes.md section 4r).  cx_h: the bandwidth h of the weights."""
    key, title = "cx", "Contextual Loss"
    params = {"cx_h": 0.5}
    taps = (contextual.TAP,)                                        # relu3_4
    needs_phase = "the contextual loss reads a tap of the VGG19 trunk, and no VGG runs in"

    def __init__(self, **kw):
        super().__init__(**kw)
        self.cx_h = float(self.cx_h)
        if not self.cx_h > 0:
            raise ValueError(f"cx_h {self.cx_h} must be > 0")

    def check(self, side, what=None):
        why = contextual.check_size(side, side)
        return why and f"--alpha_cx {self.alpha}: {what or side}, a relu3_4 tap of {'%d x %d' % contextual.tap_size(side, side)}: {why}"

    def value(self, sr, hr, taps_sr, taps_hr):
        return contextual.contextual_from_tap(taps_sr[0], taps_hr[0], self.cx_h)


TERMS = (Lpips, Ssim, Texture, Contextual)                          # the order in which the terms join the sum


def build(kw):
    """Trainer's keyword arguments of the terms -> one record per entry of TERMS, on or off, in table order; ValueError where a weight
    or a parameter is refused, TypeError for a keyword that no term takes."""
    kw = dict(kw)
    terms = [cls(**{name: kw.pop(name) for name in (cls.weight, *cls.params) if name in kw}) for cls in TERMS]
    if kw:
        raise TypeError(f"Trainer: unexpected keyword arguments {sorted(kw)}")
    return terms
