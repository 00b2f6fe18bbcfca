"""The train-step harness of the GPU tests of the optional generator-loss terms (pesr_amd/loss_terms.py): toy networks from the seeded
state dicts of tests/helpers.py, four batches of seeded images, eager runs from one start that are computed once per argument set and
shared by every test file that asks for the same harness, and a spy that records how the VGG was called.

    H = harness(seed, batch)         LR batches from seeds seed + i, HR batches from seeds seed + 10 + i, i = 0 .. 3
    H.trainer(phase, **kw)           a fresh Trainer on fresh networks; phase "pretrain" has no D and no VGG
    H.run(steps, phase, **kw)        -> (the logs of every step, the state after every step, the keyword arguments of every VGG call)
"""
import torch

from helpers import dis_sd, gen_sd, vgg_sd
from oracle import detrand

_SHARED = {}


def vgg():
    if "vgg" not in _SHARED:
        from model import VGG
        V = VGG(); V.load_state_dict(vgg_sd()); V.cuda()
        _SHARED["vgg"] = V
    return _SHARED["vgg"]


def lpips_model():
    """ONE LpipsModel.random for every run: a run's cache key holds the object."""
    if "lpips" not in _SHARED:
        import lpips_cases
        _SHARED["lpips"] = lpips_cases.model()
    return _SHARED["lpips"]


def state(tr):
    st = {"G": tr.optim_G.flat.flat_p.clone()}
    if tr.D is not None:
        st.update({"D": tr.optim_D.flat.flat_p.clone(), **{"D." + k: v.clone() for k, v in tr.D.state_dict().items()}})
    return st


def logs(d):
    return {k: v.item() for k, v in d.items()}


def step_of(tr, phase):
    return tr.gan_step if phase == "train" else tr.pretrain_step


def capture_of(tr, phase):
    return tr.capture_gan_step if phase == "train" else tr.capture_pretrain_step


class Harness:
    def __init__(self, seed, batch, ch=64, depth=2, ps=8, lr=5e-5):
        self.seed, self.batch, self.ch, self.depth, self.ps, self.lr = seed, batch, ch, depth, ps, lr
        self._data, self._runs = None, {}

    def data(self):
        if self._data is None:
            b, ps = self.batch, self.ps
            self._data = [(detrand.image_batch((b, 3, ps, ps), self.seed + i).cuda(),
                           detrand.image_batch((b, 3, 4 * ps, 4 * ps), self.seed + 10 + i).cuda()) for i in range(4)]
        return self._data

    def trainer(self, phase="train", **kw):
        from model import Discriminator, Generator
        from pesr_amd.optim import FlatAdam
        from pesr_amd.step import Trainer
        Gn = Generator({"num_channels": self.ch, "depth": self.depth, "res_scale": 0.1, "scale": 4})
        Gn.load_state_dict(gen_sd(self.ch, self.depth, 0)); Gn.cuda()
        oG = FlatAdam([p for p in Gn.parameters() if p.requires_grad], lr=self.lr, betas=(0.9, 0.999))
        if phase == "pretrain":
            return Trainer(Gn, optim_G=oG, **kw)
        D = Discriminator({"patch_size": self.ps, "spectral_norm": False}); D.load_state_dict(dis_sd(self.ps, 1)); D.cuda()
        return Trainer(Gn, D, vgg(), oG, FlatAdam(D.parameters(), lr=self.lr, betas=(0.9, 0.999)), **kw)

    def run(self, steps, phase="train", **kw):
        """Eager steps from the same start; cached per argument set."""
        key = (phase, steps, tuple(sorted(kw.items())))
        if key not in self._runs:
            tr = self.trainer(phase, **kw)
            V, calls = tr.vgg, []
            if V is not None:
                inner = V.forward

                def spy(*a, **k):
                    calls.append(dict(k))
                    return inner(*a, **k)
                V.forward = spy
            try:
                all_logs, states = [], []
                for lr, hr in self.data()[:steps]:
                    all_logs.append(logs(step_of(tr, phase)(lr, hr)))
                    states.append(state(tr))
            finally:
                if V is not None:
                    del V.forward
            self._runs[key] = (all_logs, states, calls)
        return self._runs[key]


def harness(seed, batch, **kw):
    key = ("harness", seed, batch, tuple(sorted(kw.items())))
    if key not in _SHARED:
        _SHARED[key] = Harness(seed, batch, **kw)
    return _SHARED[key]


# ---- the three properties every term has, asserted once ------------------------------------------------------------------------------------
def assert_off_is_the_step_without(H, phase, key, **kw):
    """With the term's arguments given but the term off: the logs, the states and the VGG calls of the run without them."""
    logs0, states0, calls0 = H.run(2, phase)
    logs1, states1, calls1 = H.run(2, phase, **kw)
    assert logs1 == logs0 and all(key not in l for l in logs1)
    assert calls1 == calls0 == ([{}, {}] if phase == "train" else [])  # the VGG is called without taps
    for s, s0 in zip(states1, states0):
        assert sorted(s) == sorted(s0)
        for k in s:
            assert torch.equal(s[k], s0[k]), k


def assert_only_G_moved(log1, state1, log0, state0):
    """log1 / state1: the first step with a term on; log0 / state0: without."""
    for k in log0:
        assert log1[k] == log0[k], k                                  # the other terms of the first step are what they were
    assert not torch.equal(state1["G"], state0["G"])                  # sr's gradient differs: G moved otherwise
    for k in state0:
        if k != "G":
            assert torch.equal(state1[k], state0[k]), k               # D's first step does not see the term


def assert_survives_the_capture(H, phase, keys, **kw):
    """Two eager steps, a capture, two replays: the bits of four eager steps."""
    logs4, states4, _ = H.run(4, phase, **kw)
    tr = H.trainer(phase, **kw)
    data = H.data()
    for i in range(2):
        assert logs(step_of(tr, phase)(*data[i])) == logs4[i]
    step = capture_of(tr, phase)(*data[0])
    for i in (2, 3):
        got = logs(step(*data[i]))
        assert all(k in got for k in keys) and got == logs4[i], (i, got, logs4[i])
        for k, v in state(tr).items():
            assert torch.equal(v, states4[i][k]), (i, k)
