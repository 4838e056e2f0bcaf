"""Drop-in for ``framework/model/discriminator.py`` (:4-15): ADVENT's fully convolutional discriminator, five 4x4 /
stride 2 / pad 1 convolutions with LeakyReLU(0.2) between them.  Same parameter names and shapes as the reference
(``0.weight`` ... ``8.bias``), so ``d_main`` / ``d_aux`` checkpoints interchange.

The modules are the reference's ``nn.Conv2d`` / ``nn.LeakyReLU``; only ``forward`` differs.  It runs the five layers as
``ops.disc_conv`` -- each one a space-to-depth split pass, the library's 2x2 stride-1 pre-split convolution and, on the way
back, its data / weight gradient kernels (``csrc/disc.hip``) -- when all of these hold:

* ``ONDA_DISC=hip`` is set;
* the input and every parameter live on the GPU;
* ``ops.CONV_MODE == "f16x2"`` (with the pre-split path, ``ops.H2_PATH == "dma"``);
* the input is a 4-D fp32 tensor with ``in_channels`` channels and ``H, W >= 32`` (so that the last layer still has an output).

Otherwise -- ``"f32"`` mode, the CPU, other dtypes or ranks -- it runs the module chain, as ``nn.Sequential`` does.
``ONDA_DISC=torch`` forces the module chain and is the default (a tool switch: INTEGRATION.md, "Switches"): measured on the
MI355X at 512x1024, batch 1, the HIP chain cuts the discriminator launches of an ADVENT step from 3.79 ms to 2.94 ms, and the
step (36-39 ms) is no shorter for it -- ``docs/experiments.md``, "Discriminator convolutions"."""
import os

import torch
from torch import nn

from onda_amd import ops
from onda_amd.ops import disc as odisc


class FCDiscriminator(nn.Sequential):
    def hip_path(self, x):
        """Does `forward` take the HIP chain for this input?  (module docstring)"""
        if os.environ.get("ONDA_DISC", "torch") != "hip":
            return False
        convs = [m for m in self if isinstance(m, nn.Conv2d)]
        return (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32
                and ops.CONV_MODE == "f16x2" and ops.H2_PATH == "dma"
                and x.shape[1] == convs[0].in_channels and min(x.shape[2:]) >= 32
                and all(p.is_cuda and p.dtype == torch.float32 for p in self.parameters()))

    def forward(self, x):
        if not self.hip_path(x):
            return super().forward(x)
        packs = self.__dict__.setdefault("_packs", {})
        y, slope, below = x, 1.0, None
        for i, m in enumerate(self):
            if isinstance(m, nn.LeakyReLU):
                slope = m.negative_slope
                continue
            # layer 0 reads the NCHW map; the others the NHWC output of the conv below, whose bias gradient (when it has
            # one) reads the gradient this layer hands down as fp32
            y = ops.disc_conv(y, m.weight, m.bias, slope, packs.setdefault(i, odisc.DiscPackCache()), nchw=below is None,
                              grad_f32=below is not None and below.bias is not None and below.bias.requires_grad)
            slope, below = 1.0, m
        return y.permute(0, 3, 1, 2)


def get_fc_discriminator(num_classes, ndf=64):
    widths = [num_classes, ndf, ndf * 2, ndf * 4, ndf * 8, 1]
    layers = []
    for cin, cout in zip(widths, widths[1:]):
        if layers:
            layers.append(nn.LeakyReLU(negative_slope=0.2, inplace=True))
        layers.append(nn.Conv2d(cin, cout, kernel_size=4, stride=2, padding=1))
    return FCDiscriminator(*layers)  # convolutions at 0, 2, 4, 6, 8
