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

``FusedEval(model, codes=True)`` also hands the activations from conv to conv as the consumer's low-bit codes
(one byte per element, written by the producing kernel's epilogue and read straight into the consuming kernel's
word table: cimq_module_forward_codes) wherever both layers support it; the logits are bit-identical to
``FusedEval(model)``'s, and ``fused.code_edges`` lists the edges that carried codes in the last forward.
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
    in training mode.

    ``codes=True``: an activation that only the next conv reads (``blk.conv1 -> blk.conv2``) travels as that conv's
    codes alone; one that also feeds a shortcut (``conv1 -> layer1[0].conv1``, ``blk.conv2 -> next blk.conv1``)
    travels as fp32 and codes, the fp32 for the shortcut; the last conv writes fp32 only.  An edge whose producer
    cannot write codes or whose consumer cannot read them (``Conv2dLSQCiM.codes_ready``) stays fp32.
    ``code_edges``: the (producer, consumer, kind) names of the edges that carried codes in the last forward, kind
    "codes" or "float+codes"."""

    def __init__(self, model, codes=False):
        super().__init__()
        if not isinstance(model, ResNet):
            raise TypeError("FusedEval wraps a harness.models.ResNet")
        self.model = model
        self.codes = bool(codes)
        self.code_edges = []
        self._tables = {}
        self._probe = {}
        self._chain = self._names = None

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

    def _forward_codes(self, x):
        """forward with activation codes on the conv -> conv edges (see the class)."""
        m = self.model
        if self._chain is None:
            # the convs in order, each with its BatchNorm and the block whose shortcut adds to it (None: no
            # residual); made once, the model's modules are shared, not copied
            chain = [(m.conv1, m.bn1, None)]
            for stage in (m.layer1, m.layer2, m.layer3):
                for blk in stage:
                    chain += [(blk.conv1, blk.bn1, None), (blk.conv2, blk.bn2, blk)]
            self._chain = chain
            self._names = {id(mod): name for name, mod in m.named_modules()}
        chain, names = self._chain, self._names
        self.code_edges = []
        y, q = x, None  # the current activation: fp32 (None where only codes exist) and codes for chain[i]'s conv
        block_in = None  # fp32 input of the current block, for its shortcut
        for i, (conv, bn, blk) in enumerate(chain):
            scale, shift = self.tables(bn)
            nxt = chain[i + 1][0] if i + 1 < len(chain) else None
            if i > 0 and blk is None:
                block_in = y  # conv is a block's first conv: y feeds the block's shortcut too
            residual = blk.shortcut(block_in) if blk is not None else None
            ready = getattr(conv, "fused_epilogue_ready", None)
            src = q if q is not None else y
            if ready is None or not ready(src):
                if y is None:  # (codes are handed only to a conv that was ready when they were written)
                    raise RuntimeError("FusedEval: a conv stopped taking the library path during a forward")
                y, q = self._conv(conv, bn, y, residual), None
                continue
            # codes for the next conv where this one can write them and that one can read them; the fp32 output
            # too unless the next conv is its only reader (a block's first conv)
            hand = False
            if nxt is not None and hasattr(nxt, "codes_ready"):
                # both layers are asked on every forward (a layer can leave the library path: moved, given a
                # bias, re-initialised); what is kept per input shape is only the consumer's probe, a one-byte
                # tensor viewed in the shape of its input (codes_ready looks at shape and device alone)
                key = (i, tuple(src.shape), src.device)
                probe = self._probe.get(key)
                if probe is None:
                    ho = (src.shape[2] + 2 * conv.padding[0] - conv.weight.shape[2]) // conv.stride[0] + 1
                    wo = (src.shape[3] + 2 * conv.padding[1] - conv.weight.shape[3]) // conv.stride[1] + 1
                    probe = torch.empty(1, dtype=torch.uint8, device=src.device).expand(src.shape[0], conv.out_channels,
                                                                                        ho, wo)
                    self._probe[key] = probe
                hand = conv.codes_ready(src)[1] and nxt.codes_ready(probe)[0]
            if not hand:
                y, q = conv.forward_fused(src, scale, shift, residual=residual, relu=True), None
                continue
            only_codes = chain[i + 1][2] is not None  # the next conv is a block's second: nothing else reads y
            r = conv.forward_fused(src, scale, shift, residual=residual, relu=True, out_quant=nxt,
                                   keep_float=not only_codes)
            y, q = (None, r) if only_codes else r
            self.code_edges.append((names[id(conv)], names[id(nxt)], "codes" if only_codes else "float+codes"))
        y = F.avg_pool2d(y, y.shape[3]).flatten(1)
        return m.linear(y)

    def forward(self, x):
        if torch.is_grad_enabled():
            raise RuntimeError("FusedEval is evaluation only: call it under torch.no_grad()")
        if self.codes:
            return self._forward_codes(x)
        m = self.model
        y = self._conv(m.conv1, m.bn1, x)
        for stage in (m.layer1, m.layer2, m.layer3):
            for blk in stage:
                z = self._conv(blk.conv1, blk.bn1, y)
                y = self._conv(blk.conv2, blk.bn2, z, residual=blk.shortcut(y))
        y = F.avg_pool2d(y, y.shape[3]).flatten(1)
        return m.linear(y)
