"""Drop-in for the reference's `model` package (reference model/__init__.py): the same public names,
backed by libpesr_hip.so.  `from pesr_amd.model import *` (or the top-level `model` shim) gives
Generator, Discriminator, VGG, FocalLoss and, as the reference's star-import leaks them, nn / torch / F."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .basic import BasicBlock, ChannelAttention, ChannelLayerNorm, Conv, MeanShift, PixelShuffle, ResBlock, Upsampler, WindowAttention
from .focal_loss import FocalLoss
from .pesr import Discriminator, Generator, UNetDiscriminator, attention_of_state_dict, build_discriminator, scale_of_state_dict, \
    wattn_norm_of_state_dict, wattn_of_state_dict
from .vgg import VGG

__all__ = ["Generator", "Discriminator", "UNetDiscriminator", "build_discriminator", "VGG", "FocalLoss", "Conv", "MeanShift", "BasicBlock", "ResBlock", "ChannelAttention", "WindowAttention", "ChannelLayerNorm",
           "Upsampler", "PixelShuffle", "scale_of_state_dict", "attention_of_state_dict", "wattn_of_state_dict", "wattn_norm_of_state_dict", "nn", "torch", "F"]
