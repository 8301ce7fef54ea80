"""CIFAR ResNets (He et al., option-A identity shortcuts) with the module names and parameter
layout of the reference's models/cifar10/resnet.py (conv1/bn1, layer{1,2,3}.{i}.conv{1,2}/bn{1,2},
linear), so checkpoints and state_dict keys carry over unchanged.  ``pretrained`` weights are
fetched from the network by the reference (resnet.py:127-128); here they come from a local file
(``pretrained_location`` in the prototxt) or not at all.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

__all__ = ["resnet20", "resnet32", "resnet44", "resnet56", "resnet110", "resnet1202", "ResNet", "VGG",
           "cifar10_vggsmall"]


class PadShortcut(nn.Module):
    """Option A: stride-2 subsampling plus zero channels on both sides (no parameters)."""

    def __init__(self, extra):
        super().__init__()
        self.extra = extra

    def forward(self, x):
        return F.pad(x[:, :, ::2, ::2], (0, 0, 0, 0, self.extra, self.extra))


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, cin, cout, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.shortcut = PadShortcut(cout // 4) if (stride != 1 or cin != cout) else nn.Sequential()

    def forward(self, x):
        y = F.relu(self.bn1(self.conv1(x)))
        y = self.bn2(self.conv2(y))
        return F.relu(y + self.shortcut(x))


class ResNet(nn.Module):
    def __init__(self, blocks_per_stage, num_classes=10):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 16, 3, stride=1, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(16)
        cin = 16
        stages = []
        for width, stride in ((16, 1), (32, 2), (64, 2)):
            blocks = []
            for i in range(blocks_per_stage):
                blocks.append(BasicBlock(cin, width, stride if i == 0 else 1))
                cin = width
            stages.append(nn.Sequential(*blocks))
        self.layer1, self.layer2, self.layer3 = stages
        self.linear = nn.Linear(64, num_classes)
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.kaiming_normal_(m.weight)

    def forward(self, x):
        y = F.relu(self.bn1(self.conv1(x)))
        y = self.layer3(self.layer2(self.layer1(y)))
        y = F.avg_pool2d(y, y.shape[3]).flatten(1)
        return self.linear(y)


VGG7 = (128, 128, "M", 256, 256, "M", 512, 512, "M")


class VGG(nn.Module):
    """VGG-small (VGG7) for 32 x 32 inputs with the module names of the reference's models/cifar10/vgg.py, so its
    state_dict keys load: ``features`` is one Sequential of conv (3 x 3, pad 1, no bias), BatchNorm, ReLU triples
    with a 2 x 2 max-pool after every second triple (features.0 / .1, features.3 / .4, pool at .6, ...), and
    ``classifier`` the Linear over the flattened 512 x 4 x 4 map.  Convs start from He's fan-out normal, the
    classifier from N(0, 0.01) with zero bias."""

    def __init__(self, plan=VGG7, num_classes=10):
        super().__init__()
        mods, cin, side = [], 3, 32
        for width in plan:
            if width == "M":
                mods.append(nn.MaxPool2d(kernel_size=2, stride=2))
                side //= 2
                continue
            mods += [nn.Conv2d(cin, width, 3, padding=1, bias=False), nn.BatchNorm2d(width), nn.ReLU(inplace=True)]
            cin = width
        self.features = nn.Sequential(*mods)
        self.classifier = nn.Linear(cin * side * side, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0.0, 0.01)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        return self.classifier(self.features(x).flatten(1))


def _load_pretrained(model, pretrained, pretrained_location):
    if pretrained:
        if not pretrained_location:
            raise RuntimeError("pretrained weights need a local file (pretrained_location); there is no download")
        sd = torch.load(pretrained_location, map_location="cpu", weights_only=True)
        sd = sd.get("state_dict", sd)
        model.load_state_dict({k[7:] if k.startswith("module.") else k: v for k, v in sd.items()})
    return model


def cifar10_vggsmall(pretrained=False, pretrained_location=None):
    return _load_pretrained(VGG(), pretrained, pretrained_location)


def _make(n, pretrained=False, pretrained_location=None):
    return _load_pretrained(ResNet(n), pretrained, pretrained_location)


def resnet20(pretrained=False, **kw):
    return _make(3, pretrained, **kw)


def resnet32(pretrained=False, **kw):
    return _make(5, pretrained, **kw)


def resnet44(pretrained=False, **kw):
    return _make(7, pretrained, **kw)


def resnet56(pretrained=False, **kw):
    return _make(9, pretrained, **kw)


def resnet110(pretrained=False, **kw):
    return _make(18, pretrained, **kw)


def resnet1202(pretrained=False, **kw):
    return _make(200, pretrained, **kw)
