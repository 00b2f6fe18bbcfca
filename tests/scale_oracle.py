"""CPU float64 oracle for the x2 / x3 Generator (docs/modes.md section 4e).

The reference's Generator is x4 only, so there is no golden fixture from it for these scales: the oracle is a restatement of
the EDSR-style upsampler - conv C -> r*r*C, nn.PixelShuffle(r), conv C -> 3 - in float64 torch on the CPU, composed from the
frozen oracle package (oracle.model's trunk and shapes, oracle.detrand's deterministic weights, oracle.step's train steps).
At scale 4 every function here is oracle.model's own.
"""
from collections import OrderedDict

import torch.nn.functional as F

from oracle import detrand
from oracle import model as OM
from oracle import step as OS


def generator_shapes_scaled(C, depth, scale):
    """Generator state_dict shapes in state_dict order; the upsampler keys follow Upsampler's table."""
    if scale == 4:
        return OM.generator_shapes(C, depth)
    s = OrderedDict()
    for k, v in OM.generator_shapes(C, depth).items():
        if k.startswith("upsample."):
            continue
        if k == "add_mean.weight":
            s["upsample.0.weight"], s["upsample.0.bias"] = (scale * scale * C, C, 3, 3), (scale * scale * C,)
            s["upsample.2.weight"], s["upsample.2.bias"] = (3, C, 3, 3), (3,)
        s[k] = v
    return s


def gen_sd_scaled(C, depth, scale, seed=0):
    """helpers.gen_sd at any scale: deterministic weights, fixed MeanShift entries."""
    full = generator_shapes_scaled(C, depth, scale)
    sd = detrand.fill_state_dict({k: v for k, v in full.items() if not k.startswith(("sub_mean", "add_mean"))}, seed)
    OM.set_meanshift(sd, "G")
    return {k: sd[k] for k in full}


def generator_forward_scaled(sd, x, depth, res_scale, scale):
    """oracle.model.generator_forward with the upsampler generalised: x2 / x3 = conv C -> r*r*C, pixel_shuffle(r), conv C -> 3."""
    if scale == 4:
        return OM.generator_forward(sd, x, depth, res_scale)
    x = F.conv2d(x, sd["sub_mean.weight"], sd["sub_mean.bias"])
    x = F.conv2d(x, sd["embed.weight"], sd["embed.bias"], padding=1)
    h = x
    for i in range(depth):
        r = F.conv2d(h, sd[f"body.{i}.body.0.weight"], sd[f"body.{i}.body.0.bias"], padding=1)
        r = F.relu(r)
        r = F.conv2d(r, sd[f"body.{i}.body.2.weight"], sd[f"body.{i}.body.2.bias"], padding=1)
        h = r.mul(res_scale) + h
    h = F.conv2d(h, sd[f"body.{depth}.weight"], sd[f"body.{depth}.bias"], padding=1)
    h = h + x
    h = F.conv2d(h, sd["upsample.0.weight"], sd["upsample.0.bias"], padding=1)
    h = F.pixel_shuffle(h, scale)
    h = F.conv2d(h, sd["upsample.2.weight"], sd["upsample.2.bias"], padding=1)
    return F.conv2d(h, sd["add_mean.weight"], sd["add_mean.bias"])


class ScaledTrainState(OS.TrainState):
    """oracle.step.TrainState whose G is the scaled Generator (cfg["scale"]); OS.gan_step / OS.pretrain_step work unchanged."""

    def G(self, x):
        return generator_forward_scaled(self.g, x, self.cfg["depth"], self.cfg["res_scale"], self.cfg.get("scale", 4))
