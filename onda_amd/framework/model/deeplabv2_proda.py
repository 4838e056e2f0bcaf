"""Drop-in for the reference's ``framework/model/deeplabv2_proda.py``: the DeepLabV2 / ResNet-101 of ProDA, the fourth name of
the reference's ``MODEL_NAMES`` (``DeepLabv2-Resnet101-ProDA``), executed by the gfx950 kernels of ``libonda_hip.so``.

What is kept from the reference: ``Deeplab(BatchNorm, num_classes=21, freeze_bn=False, restore_from=None, initialization=None,
bn_clr=False)`` and ``ResNet101(block, layers, num_classes, BatchNorm, bn_clr=False)``; the module tree, so ``state_dict()`` has
the same 653 keys in the same order, all 341 parameters trainable -- the affine parameters of all 104 BatchNorms included, which
is what the blocks of ``deeplabv2.py`` never are; the construction order and init recipe (the loops over ``conv2d_list`` look at
``nn.Sequential`` wrappers and initialise nothing, the final ``modules()`` loop gives every conv weight ``normal_(0, 0.01)``), so a
torch seed produces the reference's initial weights; ``forward(x, ssl=False, lbl=None) -> (None, {"feat", "out"})``; the nested walk
of ``get_1x_lr_params`` / ``get_10x_lr_params`` / ``optim_parameters`` (942 entries over 312 tensors and 29 entries: ``ReplaySGD``
replays the multiplicities) and ``adjust_learning_rate``.  ``layer5`` is the main head here; there is no ``layer6``.

What is different.  NO NETWORK, EVER: where the reference calls ``model_zoo.load_url`` (``initialization is None``) this module
looks for ``resnet101-5d3b4d8f.pth`` in ``torch.hub.get_dir()/checkpoints`` -- where a cached download of the reference lies --
loads its matching keys if it is there, and otherwise keeps the seeded init with one warning that names the file.  ``bn_clr=True``
(a BatchNorm with no convolution in front; the handler never sets it) raises NotImplementedError.  The blocks, the head, the stem,
the weight packer and the gradient sinks are those of ``deeplabv2.py``: train-mode BatchNorms hand dgamma / dbeta out of the
backward sums they reduce anyway (``ops.BNTrainLimbFn`` / ``BNPairLimbFn`` / ``BNTrainFn``); ``freeze_bn=True`` models run the frozen
routes untouched.  One GPU only while a BatchNorm affine parameter trains (``deeplabv2.require_single_gpu_affine``).
"""
import os
import warnings

import torch
import torch.nn as nn

from onda_amd import ops
from onda_amd.framework.model.deeplabv2 import (Bottleneck as _Block, Classifier_Module2, HipBatchNorm2d, HipConv2d, ResNetMulti,
                                                affine_par)

PRETRAINED_FILE = "resnet101-5d3b4d8f.pth"


def _hip_norm(BatchNorm):
    return HipBatchNorm2d if BatchNorm is nn.BatchNorm2d else BatchNorm


class Bottleneck(_Block):
    """``deeplabv2.Bottleneck`` with the reference's signature here (``BatchNorm=``): every BatchNorm of the block trains."""

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, BatchNorm=None):
        super().__init__(inplanes, planes, stride, dilation=dilation, downsample=downsample, norm_module=_hip_norm(BatchNorm),
                         norm_grad=True)


class ResNet101(ResNetMulti):
    """The stem, ``_stem_train``, ``__deepcopy__`` and the packer handling are ResNetMulti's; the tree, the forward and the
    parameter groups are the reference's ResNet101."""
    main_head = "layer5"
    feat = True

    def __init__(self, block, layers, num_classes, BatchNorm, bn_clr=False):
        if bn_clr:
            raise NotImplementedError("onda_amd: bn_clr=True puts a BatchNorm behind layer4 with no convolution in front of it; "
                                      "the HIP path has no such site (the reference's handler never sets it)")
        BatchNorm = _hip_norm(BatchNorm)
        if not (isinstance(BatchNorm, type) and issubclass(BatchNorm, HipBatchNorm2d)):
            raise NotImplementedError("onda_amd: the ProDA ResNet-101 runs on BatchNorm2d (torch.nn.BatchNorm2d or HipBatchNorm2d)")
        nn.Module.__init__(self)
        self.inplanes = 64
        self.bn_clr = bn_clr
        self.multi_level = False
        self.conv1 = HipConv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = BatchNorm(64, affine=affine_par)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1, ceil_mode=True)
        self.layer1 = self._make_layer(block, 64, layers[0], BatchNorm=BatchNorm)
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2, BatchNorm=BatchNorm)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=1, dilation=2, BatchNorm=BatchNorm)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=1, dilation=4, BatchNorm=BatchNorm)
        self.layer5 = self._make_pred_layer(Classifier_Module2, 2048, [6, 12, 18, 24], [6, 12, 18, 24], num_classes)
        for m in self.modules():  # (this also overrides the head's own init of its conv weights)
            if isinstance(m, nn.Conv2d):
                m.weight.data.normal_(0, 0.01)
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()

    def _make_layer(self, block, planes, blocks, stride=1, dilation=1, BatchNorm=None):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion or dilation == 2 or dilation == 4:
            downsample = nn.Sequential(
                HipConv2d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                BatchNorm(planes * block.expansion, affine=affine_par))
        layers = [block(self.inplanes, planes, stride, dilation=dilation, downsample=downsample, BatchNorm=BatchNorm)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes, dilation=dilation, BatchNorm=BatchNorm))
        return nn.Sequential(*layers)

    def _make_pred_layer(self, block, inplanes, dilation_series, padding_series, num_classes):
        return block(inplanes, dilation_series, padding_series, num_classes)

    def forward(self, x, ssl=False, lbl=None):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected an image batch f32[B,3,H,W], got {tuple(x.shape)}")
        ops._require_cuda(x, "image batch")
        x = x.to(torch.float32)
        packer = self.__dict__.get("_packer")
        if packer is None:
            # every convolution but the stem (its own im2col route) and the class head (packed at its padded width)
            plain = [m for name, m in self.named_modules() if isinstance(m, HipConv2d) and m is not self.conv1
                     and not name.endswith("head.1")]
            packer = self.__dict__["_packer"] = ops.ModelPacker(plain)
        packer.refresh(need_dgrad=torch.is_grad_enabled() and self.training)
        y = self._stem(x)
        y = self.layer1(y)
        y = self.layer2(y)
        y = self.layer3(y)
        y = self.layer4(y)
        return None, self.layer5(y, get_feat=True)

    # ---- parameter groups: the reference's nested walk, duplicates included -----------------------------------------------------
    def get_1x_lr_params(self):
        for top in (self.conv1, self.bn1, self.layer1, self.layer2, self.layer3, self.layer4):
            for mod in top.modules():
                for p in mod.parameters():
                    if p.requires_grad:
                        yield p

    def get_10x_lr_params(self):
        for p in self.layer5.parameters():
            yield p

    def optim_parameters(self, lr):
        return [{"params": self.get_1x_lr_params(), "lr": lr}, {"params": self.get_10x_lr_params(), "lr": 10 * lr}]

    def adjust_learning_rate(self, args, optimizer, i):
        lr = args.learning_rate * ((1 - float(i) / args.num_steps) ** (args.power))
        optimizer.param_groups[0]["lr"] = lr
        if len(optimizer.param_groups) > 1:
            optimizer.param_groups[1]["lr"] = lr * 10


def freeze_bn_func(m):
    if m.__class__.__name__.find("BatchNorm") != -1 or isinstance(m, nn.BatchNorm2d):
        m.weight.requires_grad = False
        m.bias.requires_grad = False


def pretrained_path():
    """Where a cached download of the reference's ImageNet weights lies: ``torch.hub.get_dir()/checkpoints/resnet101-5d3b4d8f.pth``."""
    return os.path.join(torch.hub.get_dir(), "checkpoints", PRETRAINED_FILE)


def _load_matching(model, pretrain_dict):
    state_dict = model.state_dict()
    state_dict.update({k: v for k, v in pretrain_dict.items() if k in state_dict})
    model.load_state_dict(state_dict)


def Deeplab(BatchNorm, num_classes=21, freeze_bn=False, restore_from=None, initialization=None, bn_clr=False):
    model = ResNet101(Bottleneck, [3, 4, 23, 3], num_classes, BatchNorm, bn_clr=bn_clr)
    if freeze_bn:
        model.apply(freeze_bn_func)
    if initialization is None:
        path = pretrained_path()
        if os.path.isfile(path):
            _load_matching(model, torch.load(path, map_location="cpu"))
        else:
            warnings.warn(f"onda_amd: {PRETRAINED_FILE} is not in {os.path.dirname(path)} and nothing is ever downloaded: the model "
                          f"keeps its seeded initialisation (put the file there, or pass initialization= / restore_from=)")
    else:
        _load_matching(model, torch.load(initialization, map_location="cpu")["state_dict"])
    if restore_from is not None:
        checkpoint = torch.load(restore_from, map_location="cpu")
        model.load_state_dict(checkpoint["ResNet101"]["model_state"])
    return model
