"""Evaluation of a harness ResNet with each BatchNorm folded into a per-channel affine and, together with
the residual add and the ReLU, applied inside the CiM conv's forward kernel
(``Conv2dLSQCiM.forward_fused`` -> cimq_module_forward_epilogue): one library launch per conv where
``ResNet.forward`` runs the conv and five or six elementwise torch kernels.

    fused = FusedEval(model)        # shares the model's modules, copies no parameter
    with torch.no_grad():
        logits = fused(x)

The folded network is NOT bit-identical to the BatchNorm one: ``(v - mean) / sqrt(var + eps) * gamma + beta``
and ``v * scale + shift`` round differently, and a last-bit difference in front of an activation quantiser can
move a code.  It IS bit-identical to the same folded arithmetic written in torch (the tests' twin).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .models import ResNet

__all__ = ["fold_bn", "FusedEval"]


def fold_bn(bn):
    """(scale, shift) of a BatchNorm2d in evaluation mode, ``bn(v) ~ v * scale[c] + shift[c]``: computed in
    fp64 from the module's fp32 tensors and rounded once to fp32.  scale = gamma / sqrt(running_var + eps),
    shift = beta - running_mean * scale; a non-affine BN has gamma = 1, beta = 0."""
    if bn.running_mean is None or bn.running_var is None:
        raise RuntimeError("fold_bn needs a BatchNorm that tracks running statistics")
    mean, var = bn.running_mean.detach().double(), bn.running_var.detach().double()
    gamma = bn.weight.detach().double() if bn.weight is not None else torch.ones_like(var)
    beta = bn.bias.detach().double() if bn.bias is not None else torch.zeros_like(var)
    s = gamma / torch.sqrt(var + bn.eps)
    return s.float().contiguous(), (beta - mean * s).float().contiguous()


def _bn_versions(bn):
    return tuple(None if t is None else (t._version, t.data_ptr(), t.device)
                 for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))


class FusedEval(nn.Module):
    """Evaluation-only forward of a ``harness.models.ResNet``: conv1 and each block's two convs run
    ``forward_fused`` with their BatchNorm folded (fold_bn), the block's shortcut as the second conv's residual
    and the ReLU in the epilogue; pooling and the classifier as ``ResNet.forward``.  A conv that is not a
    Conv2dLSQCiM on the library path (not replaced, adcbits 0, bias set, CPU tensors) runs as ``conv(x)``
    followed by the same four torch operations.  The folded tables are kept per BatchNorm and remade when the
    version of gamma, beta, running_mean or running_var changes.  Raises under grad mode or with a BatchNorm
    in training mode."""

    def __init__(self, model):
        super().__init__()
        if not isinstance(model, ResNet):
            raise TypeError("FusedEval wraps a harness.models.ResNet")
        self.model = model
        self._tables = {}

    def tables(self, bn):
        if bn.training:
            raise RuntimeError("FusedEval: BatchNorm in training mode (call model.eval() first)")
        key = _bn_versions(bn)
        hit = self._tables.get(id(bn))
        if hit is None or hit[0] != key:
            hit = (key, fold_bn(bn))
            self._tables[id(bn)] = hit
        return hit[1]

    def _conv(self, conv, bn, x, residual=None):
        scale, shift = self.tables(bn)
        ready = getattr(conv, "fused_epilogue_ready", None)
        if ready is not None and ready(x):
            return conv.forward_fused(x, scale, shift, residual=residual, relu=True)
        y = conv(x) * scale.view(1, -1, 1, 1)
        y = y + shift.view(1, -1, 1, 1)
        if residual is not None:
            y = y + residual
        return torch.relu(y)

    def forward(self, x):
        if torch.is_grad_enabled():
            raise RuntimeError("FusedEval is evaluation only: call it under torch.no_grad()")
        m = self.model
        y = self._conv(m.conv1, m.bn1, x)
        for stage in (m.layer1, m.layer2, m.layer3):
            for blk in stage:
                z = self._conv(blk.conv1, blk.bn1, y)
                y = self._conv(blk.conv2, blk.bn2, z, residual=blk.shortcut(y))
        y = F.avg_pool2d(y, y.shape[3]).flatten(1)
        return m.linear(y)
