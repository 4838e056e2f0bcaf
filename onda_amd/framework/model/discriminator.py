"""Drop-in for ``framework/model/discriminator.py`` (:4-15): ADVENT's fully convolutional discriminator, five 4x4 /
stride 2 / pad 1 convolutions with LeakyReLU(0.2) between them.  Same parameter names and shapes as the reference
(``0.weight`` ... ``8.bias``), so ``d_main`` / ``d_aux`` checkpoints interchange.

Plain ``torch.nn``: ``ops/conv.py`` has a strided data gradient for 1x1 kernels only, and these layers need one for 4x4.
The discriminator's input -- the entropy map -- is where this method's HIP kernel sits (``ops.upsample_entropy``)."""
from torch import nn


def get_fc_discriminator(num_classes, ndf=64):
    widths = [num_classes, ndf, ndf * 2, ndf * 4, ndf * 8, 1]
    layers = []
    for cin, cout in zip(widths, widths[1:]):
        if layers:
            layers.append(nn.LeakyReLU(negative_slope=0.2, inplace=True))
        layers.append(nn.Conv2d(cin, cout, kernel_size=4, stride=2, padding=1))
    return nn.Sequential(*layers)  # convolutions at 0, 2, 4, 6, 8
