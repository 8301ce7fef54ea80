"""Evaluation of a harness ResNet (or VGG: ``FusedEval._forward_vgg``) with each BatchNorm folded into a per-channel
affine and, together with the residual add and the ReLU, applied inside the CiM conv's forward kernel
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

from .models import VGG, ResNet

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


def _out_shape(conv, in_shape):
    """NCHW output shape of the CiM conv ``conv`` for input shape ``in_shape``."""
    from ..functional import conv_out_hw
    return (in_shape[0], conv.out_channels) + conv_out_hw(in_shape[2], in_shape[3], *conv.weight.shape[2:],
                                                          conv.stride, conv.padding)


def assign_slots(steps):
    """Activation slots by liveness.  ``steps``: the plan in execution order, each ``(reads, write)`` -- the values
    the step reads and the one it writes (None: the head).  Returns ``({value: slot}, n_slots)``: a value keeps its
    slot until its last reader has run, a step's output never takes the slot of a value that step reads, and the
    lowest free slot is taken -- so the peak is the largest number of values alive at once, not one per layer.
    Values that no step writes (the net's input) get no slot."""
    last = {}
    for t, (reads, write) in enumerate(steps):
        for v in reads:
            last[v] = t
        if write is not None:
            last.setdefault(write, t)
    slot_of, holder = {}, []  # holder[s]: the value in slot s
    for t, (reads, write) in enumerate(steps):
        if write is None:
            continue
        free = [s for s, v in enumerate(holder) if last[v] < t]
        if free:
            s = free[0]
            holder[s] = write
        else:
            s = len(holder)
            holder.append(write)
        slot_of[write] = s
    return slot_of, len(holder)


def resnet_steps(blocks_per_stage):
    """``assign_slots``' steps of a harness ResNet run as one cimq_net_forward plan: value i is conv i's output, a
    block's second conv also reads the block's input (the shortcut is a view of it, not a tensor of its own), the
    head reads the last conv's."""
    steps = [((), 0)]  # conv1 reads x
    v = 0
    for _ in range(3 * blocks_per_stage):
        steps.append(((v,), v + 1))          # blk.conv1
        steps.append(((v + 1, v), v + 2))    # blk.conv2 + shortcut(block input)
        v += 2
    steps.append(((v,), None))
    return steps


class _NetPlan:
    """One cimq_net_forward plan of a FusedEval: the ctypes structures, everything they point to (kept alive here)
    and the arena behind the slots.  ``run(x)`` is one library call."""

    def __init__(self, fused, x):
        from .. import _lib
        from .models import PadShortcut
        m = fused.model
        chain, names = fused._chain_of()
        dev = x.device
        self.keep = []
        self.code_edges = []
        n = len(chain)
        steps = resnet_steps(len(m.layer1))
        if len(steps) != n + 1:
            raise _NoPlan("the model is not three equal stages of basic blocks")
        slot_of, n_slots = assign_slots(steps)
        layers = (_lib.NetLayer * n)()
        shape = tuple(x.shape)
        shapes, block_shape = [], None
        for i, (conv, bn, blk) in enumerate(chain):
            L = layers[i]
            self._fill_layer(fused, L, conv, bn, shape, dev)
            L.in_slot = -1 if i == 0 else slot_of[i - 1]
            L.out_slot = slot_of[i]
            if i > 0 and blk is None:
                block_shape = shape  # a block's first conv: its input feeds the block's shortcut too
            out_shape = _out_shape(conv, shape)
            if blk is not None:  # the shortcut: the block's input (value i - 2) as a view
                L.res_slot = slot_of[i - 2]
                if isinstance(blk.shortcut, PadShortcut):
                    L.res_c0, L.res_stride = int(blk.shortcut.extra), 2
                elif isinstance(blk.shortcut, nn.Sequential) and len(blk.shortcut) == 0:
                    if tuple(block_shape) != out_shape:
                        raise _NoPlan("an identity shortcut of another shape")
                else:
                    raise _NoPlan("a shortcut that is neither the identity nor option A")
            shapes.append((shape, out_shape))
            shape = out_shape
        if shape[2] != shape[3]:
            raise _NoPlan("the final map is not square (ResNet.forward pools with kernel W)")
        # activation codes on the conv -> conv edges, by FusedEval's edge rules
        if fused.codes:
            for i in range(n - 1):
                conv, nxt = chain[i][0], chain[i + 1][0]
                pin = torch.empty(1, dtype=torch.uint8, device=dev).expand(shapes[i][0])
                pout = torch.empty(1, dtype=torch.uint8, device=dev).expand(shapes[i][1])
                if not (conv.codes_ready(pin)[1] and nxt.codes_ready(pout)[0]):
                    continue
                only_codes = chain[i + 1][2] is not None  # the next conv is a block's second: nothing else reads y
                layers[i].out_mode, layers[i].consumer = (2 if only_codes else 3), i + 1
                layers[i + 1].in_codes = 1
                self.code_edges.append((names[id(conv)], names[id(nxt)], "codes" if only_codes else "float+codes"))
        lin = m.linear
        if not isinstance(lin, nn.Linear) or lin.weight.device != dev or lin.weight.dtype != torch.float32 or \
                not lin.weight.is_contiguous() or lin.in_features != shape[1]:
            raise _NoPlan("the classifier is not a contiguous fp32 nn.Linear over the last conv's channels")
        self._finish(layers, n_slots, slot_of[n - 1], lin, x, shape)

    def _fill_layer(self, fused, L, conv, bn, shape, dev):
        """one conv of the plan for input ``shape``: its descriptors, prepared weight side, ctx and folded BatchNorm
        (kept alive on the plan), an fp32 output with ReLU and no residual; the caller sets the slots"""
        import ctypes

        from .. import _lib
        from .. import functional as CF
        probe = torch.empty(1, dtype=torch.uint8, device=dev).expand(shape)
        if not getattr(conv, "fused_epilogue_ready", lambda t: False)(probe):
            raise _NoPlan("a conv is off the library path")
        if conv.stochastic_quant:
            raise _NoPlan("stochastic-ADC layers run in the loop")
        # (a shift-ADC layer that is ready is one the fused shift path takes: its prepared side carries beta_cim)
        ps = (conv.weight, conv.alpha_act, conv.alpha_weight, conv.alpha_cim) + \
            ((conv.beta_cim,) if conv.adc_shift else ())
        if any(t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev) for t in ps):
            raise _NoPlan("parameters must be contiguous fp32 on the input's device")
        if conv.binary_mask.device != dev:
            conv.binary_mask = conv.binary_mask.to(dev)
        desc, lsq = CF.module_descs(conv, shape, inference=True)
        wp = conv._inf_prep = CF.inference_weights(conv, shape, conv._inf_prep)
        lsq.wprep = wp.buf.data_ptr()
        sizes = _lib.query_sizes(desc)
        ctx = torch.empty(max(sizes.module_ctx_bytes, 1), device=dev, dtype=torch.uint8)
        bm = conv.binary_mask.to(device=dev, dtype=torch.int8).contiguous()
        sg = conv.signed_act.detach().to(device=dev, dtype=torch.float32).reshape(-1)[:1].contiguous()
        scale, shift = fused.tables(bn)
        scale, shift = scale.to(dev), shift.to(dev)
        self.keep += [desc, lsq, wp, ctx, bm, sg, scale, shift]
        L.desc, L.lsq = ctypes.pointer(desc), ctypes.pointer(lsq)
        L.weight, L.alpha_act = conv.weight.data_ptr(), conv.alpha_act.data_ptr()
        L.alpha_weight = conv.alpha_weight.data_ptr()
        L.alpha_cim = None if conv.alpha_cim is None else conv.alpha_cim.data_ptr()
        L.beta_cim = conv.beta_cim.data_ptr() if conv.adc_shift else None
        L.binary_mask, L.signed_act = bm.data_ptr(), sg.data_ptr()
        L.scale, L.shift, L.epi_flags = scale.data_ptr(), shift.data_ptr(), _lib.CIMQ_EPI_RELU
        L.out_mode, L.consumer, L.in_codes = 1, 0, 0
        L.res_slot, L.res_c0, L.res_stride, L.reserved = -1, 0, 1, 0
        L.ctx = ctx.data_ptr()
        return desc

    def _finish(self, layers, n_slots, last_slot, lin, x, shape, ext=None):
        """the head over ``lin``, the plan's sizes (``ext``: a ``_lib.NetExt``, kept) and the arena behind its slots"""
        import ctypes

        from .. import _lib
        from .. import functional as CF
        n, dev = len(layers), x.device
        head = _lib.NetHead()
        head.in_slot, head.classes = last_slot, lin.out_features
        head.weight = lin.weight.data_ptr()
        head.bias = None if lin.bias is None else lin.bias.data_ptr()
        head.pooled = None
        net = _lib.NetDesc()
        net.n_layers, net.n_slots = n, n_slots
        net.layers, net.head = layers, ctypes.pointer(head)
        net.B, net.C, net.H, net.W = x.shape
        self.keep += [layers, head]
        self.ext = ext
        try:
            fb, cb, wsb = CF.net_sizes(net, ext)
        except _lib.CimqError as e:
            raise _NoPlan(str(e))
        # one arena behind the slots' planes and the shared workspace
        al = lambda v: (v + 255) & ~255  # noqa: E731
        total = sum(al(v) for v in fb) + sum(al(v) for v in cb) + al(wsb)
        self.arena = torch.empty(max(total, 256), device=dev, dtype=torch.uint8)
        base, off = self.arena.data_ptr(), 0
        if base % 256:
            raise _NoPlan("the arena is not 256-byte aligned")
        self.slot_float, self.slot_codes = (ctypes.c_void_p * n_slots)(), (ctypes.c_void_p * n_slots)()
        self._float_off = []
        for s in range(n_slots):
            self.slot_float[s] = base + off if fb[s] else None
            self._float_off.append(off)
            off += al(fb[s])
        for s in range(n_slots):
            self.slot_codes[s] = base + off if cb[s] else None
            off += al(cb[s])
        self.ws = base + off
        self.net, self.n_slots, self.classes, self.batch = net, n_slots, lin.out_features, x.shape[0]
        self.last_shape, self.last_slot = shape, last_slot
        self._run = CF.net_forward

    def run(self, x):
        logits = torch.empty(self.batch, self.classes, device=x.device, dtype=torch.float32)
        self._run(self.net, x.data_ptr(), self.slot_float, self.slot_codes, logits.data_ptr(), self.ws,
                  torch.cuda.current_stream(x.device).cuda_stream, self.ext)
        return logits

    def last_plane(self):
        """the last conv's fp32 output as the last run left it in the arena (a view, overwritten by the next run)"""
        nb = 4 * self.last_shape[0] * self.last_shape[1] * self.last_shape[2] * self.last_shape[3]
        o = self._float_off[self.last_slot]
        return self.arena[o:o + nb].view(torch.float32).view(self.last_shape)


def _is_pool2(mod):
    """an ``nn.MaxPool2d`` that is exactly the 2 x 2 / stride-2 pool a conv's kernel can apply to its own output"""
    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)  # noqa: E731
    return (isinstance(mod, nn.MaxPool2d) and pair(mod.kernel_size) == (2, 2) and pair(mod.stride) == (2, 2) and
            pair(mod.padding) == (0, 0) and pair(mod.dilation) == (1, 1) and not mod.ceil_mode and
            not mod.return_indices)


def _vgg_triples(model):
    """``[(k, conv, bn, pooled)]`` of a harness VGG's ``features``: conv k with the BatchNorm and ReLU behind it, and
    whether a 2 x 2 max-pool (``_is_pool2``) follows them; None where ``features`` holds anything else"""
    mods, out, i = list(model.features), [], 0
    is_conv = lambda mod: isinstance(mod, nn.Conv2d) or hasattr(mod, "forward_fused")  # noqa: E731
    while i < len(mods):
        if not (is_conv(mods[i]) and i + 2 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm2d) and
                isinstance(mods[i + 2], nn.ReLU)):
            return None
        pooled = i + 3 < len(mods) and _is_pool2(mods[i + 3])
        out.append((i, mods[i], mods[i + 1], pooled))
        i += 4 if pooled else 3
    return out


class _VggPlan(_NetPlan):
    """The cimq_net_forward_ex plan of a harness VGG under ``FusedEval(pool=True, net=True)``: the convs of
    ``features`` in order on fp32 edges, a straight chain's slots, each 2 x 2 max-pool applied by the conv in front of
    it (``cimq_net_ext.pool``) and ``classifier`` as the flatten head.  ``pooled``: those convs' names."""

    def __init__(self, fused, x):
        from .. import _lib
        m, dev = fused.model, x.device
        self.keep, self.code_edges, self.pooled = [], [], []
        triples = _vgg_triples(m)
        if not triples:
            raise _NoPlan("features is not a sequence of conv, BatchNorm, ReLU triples and 2 x 2 max-pools")
        n = len(triples)
        slot_of, n_slots = assign_slots([((), 0)] + [((i - 1,), i) for i in range(1, n)] + [((n - 1,), None)])
        layers = (_lib.NetLayer * n)()
        pool, shape = [0] * n, tuple(x.shape)
        for i, (k, conv, bn, pooled) in enumerate(triples):
            L = layers[i]
            desc = self._fill_layer(fused, L, conv, bn, shape, dev)
            L.in_slot = -1 if i == 0 else slot_of[i - 1]
            L.out_slot = slot_of[i]
            in_shape, shape = shape, _out_shape(conv, shape)
            if pooled:
                if not conv.pool_ready(torch.empty(1, dtype=torch.uint8, device=dev).expand(in_shape)):
                    route = _lib.ROUTE_NAMES.get(_lib.module_route(desc)[0], "?")
                    why = "it is off the wide route (its forward route is %s)" % route if route != "wide" else \
                        "its output is wider than 32 columns"
                    raise _NoPlan("features.%d: the max-pool behind it cannot run in its kernel: %s" % (k, why))
                pool[i] = _lib.CIMQ_POOL_MAX2
                self.pooled.append("features.%d" % k)
                shape = shape[:2] + (shape[2] // 2, shape[3] // 2)
        lin = m.classifier
        if not isinstance(lin, nn.Linear) or lin.weight.device != dev or lin.weight.dtype != torch.float32 or \
                not lin.weight.is_contiguous() or lin.in_features != shape[1] * shape[2] * shape[3]:
            raise _NoPlan("the classifier is not a contiguous fp32 nn.Linear over the flattened last map")
        self._finish(layers, n_slots, slot_of[n - 1], lin, x, shape,
                     _lib.make_net_ext(pool, _lib.NET_HEAD_FLATTEN))


class _NoPlan(Exception):
    """why a FusedEval(net=True) forward runs the loop instead"""


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
    "codes" or "float+codes".

    ``net=True``: the whole forward is one library call (cimq_net_forward): the convs with the same arguments and
    edge rules as the loop, each option-A shortcut read as a view of the block's input inside the epilogue of the
    conv it adds to, and pooling + classifier in one head kernel -- no torch kernel, no Python between the launches.
    The plan (descriptors, prepared weight sides, folded tables, ctx buffers, one arena behind the activation slots,
    which are assigned by liveness: ``assign_slots``) is built once and reused while its key matches (``_net_state``).
    Every conv's output is bit for bit the loop's; the logits differ from the loop's by the summation order of the
    pooling and of the classifier alone.  Shift-ADC layers (``adc_shift``) on the fused shift path are plan layers
    like any other; stochastic-ADC layers run in the loop.  Where a conv is off the library path, the library refuses the plan or the
    final map is not square, the loop runs: ``net_used`` says which of the two the last forward was.

    ``pool=True`` (a VGG; a ResNet has nothing to pool): a conv whose ReLU is followed by ``nn.MaxPool2d(2, 2)`` and
    whose ``pool_ready`` holds stores the pooled plane itself (``forward_fused(pool=2)``, bit for bit the torch pool
    of its output) and the torch pool is skipped; ``pooled`` lists the convs that did.  With ``net=True`` as well the
    VGG is one cimq_net_forward_ex call: the convs of ``features`` on fp32 edges, each pool in the conv in front of it
    and ``classifier`` as the head over the flattened map (``_VggPlan``; the plan is kept under the same key).  A pool
    behind a conv that cannot pool in its kernel means no plan: the loop runs and ``net_reason`` names the layer."""

    def __init__(self, model, codes=False, net=False, pool=False):
        super().__init__()
        if not isinstance(model, (ResNet, VGG)):
            raise TypeError("FusedEval wraps a harness.models.ResNet or a harness.models.VGG")
        self.model = model
        self.codes = bool(codes)
        self.net = bool(net)
        self.pool = bool(pool)  # a VGG's 2 x 2 max-pools in the kernel of the conv in front of them (see _forward_vgg)
        self.pooled = []        # the names of the convs that pooled their own output in the last forward
        self.net_used = False   # whether the last forward ran as one cimq_net_forward call
        self.net_reason = None  # ... and if not, why (the loop ran)
        self.code_edges = []
        self._tables = {}
        self._probe = {}
        self._chain = self._names = None
        self._net_key = self._net_plan = None

    def _chain_of(self):
        """the convs in order, each with its BatchNorm and the block whose shortcut adds to it (None: no residual),
        and the module names; made once, the model's modules are shared, not copied"""
        if self._chain is None:
            m = self.model
            if isinstance(m, VGG):  # (a straight chain: no residuals)
                chain = [(conv, bn, None) for _, conv, bn, _ in _vgg_triples(m) or ()]
            else:
                chain = [(m.conv1, m.bn1, None)]
                for stage in (m.layer1, m.layer2, m.layer3):
                    for blk in stage:
                        chain += [(blk.conv1, blk.bn1, None), (blk.conv2, blk.bn2, blk)]
            self._chain = chain
            self._names = {id(mod): name for name, mod in m.named_modules()}
        return self._chain, self._names

    def _net_state(self, x):
        """the key a plan is reused under: the input's shape and device, whether edges carry codes, and the
        (_version, data_ptr) of every conv parameter (a shift layer's beta_cim among them), BatchNorm tensor and
        classifier tensor; None where a conv is
        off the library path (the loop then runs, and says so)"""
        from ..functional import _versions
        chain, _ = self._chain_of()
        key = [tuple(x.shape), x.device, self.codes, self.pool]
        for conv, bn, _ in chain:
            ready = getattr(conv, "fused_epilogue_ready", None)
            if ready is None or not ready(x):
                return None
            if bn.training:
                raise RuntimeError("FusedEval: BatchNorm in training mode (call model.eval() first)")
            key.append(_versions(conv.weight, conv.alpha_act, conv.alpha_weight, conv.alpha_cim, conv.binary_mask,
                                 conv.signed_act, getattr(conv, "beta_cim", None)))
            key.append(_bn_versions(bn))
        lin = self.model.classifier if isinstance(self.model, VGG) else self.model.linear
        key.append(_versions(getattr(lin, "weight", None), getattr(lin, "bias", None)))
        return tuple(key)

    def _forward_net(self, x):
        """the forward as one library call, or None where the loop has to run (``net_reason`` says why)"""
        if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4):
            self.net_reason = "not a ROCm NCHW input"
            return None
        key = self._net_state(x)
        if key is None:
            self.net_reason = "a conv is off the library path"
            return None
        if key != self._net_key:
            self._net_key, self._net_plan = key, None
            try:
                self._net_plan = (_VggPlan if isinstance(self.model, VGG) else _NetPlan)(self, x)
                self.net_reason = None
            except _NoPlan as e:
                self.net_reason = str(e)
        plan = self._net_plan
        if plan is None:
            return None
        xc = x if (x.dtype == torch.float32 and x.is_contiguous() and x.data_ptr() % 16 == 0) else \
            x.to(torch.float32).contiguous().clone()
        y = plan.run(xc)
        self.code_edges = list(plan.code_edges)
        self.pooled = list(getattr(plan, "pooled", ()))
        return y

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
        chain, names = self._chain_of()
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
                    probe = torch.empty(1, dtype=torch.uint8, device=src.device).expand(_out_shape(conv, src.shape))
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

    def _forward_vgg(self, x):
        """A ``harness.models.VGG``: every conv of ``features`` runs ``forward_fused`` with the BatchNorm behind it
        folded and the ReLU in the epilogue; the max-pools, the flatten and the classifier stay torch operations.
        ``codes=True``: a conv whose only reader is the next conv hands it codes alone where ``codes_ready`` says the
        producer writes and the consumer reads them -- the rule of ``_forward_codes``; an edge into a max-pool stays
        fp32.  In VGG7 every such consumer has 128 channels or more (the wide route, which reads no codes), so all
        its edges stay fp32; a narrower ``VGG(plan=...)`` gets code edges."""
        mods = list(self.model.features)
        names = {id(mod): "features.%d" % k for k, mod in enumerate(mods)}
        is_conv = lambda mod: isinstance(mod, nn.Conv2d) or hasattr(mod, "forward_fused")  # noqa: E731
        self.code_edges, self.pooled = [], []
        y, i = x, 0  # y: the current activation, fp32 or (handed by the conv before) the consumer's codes
        while i < len(mods):
            mod = mods[i]
            if not is_conv(mod):
                y = mod(y)
                i += 1
                continue
            if not (i + 2 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm2d) and isinstance(mods[i + 2], nn.ReLU)):
                raise RuntimeError("FusedEval: a VGG conv without its BatchNorm and ReLU behind it")
            bn = mods[i + 1]
            # pool=True: the 2 x 2 max-pool behind the ReLU runs in this conv's kernel where the layer can (pool_ready)
            if self.pool and i + 3 < len(mods) and _is_pool2(mods[i + 3]) and y.dtype != torch.uint8 and \
                    hasattr(mod, "pool_ready") and mod.pool_ready(y):
                scale, shift = self.tables(bn)
                y = mod.forward_fused(y, scale, shift, relu=True, pool=2)
                self.pooled.append(names[id(mod)])
                i += 4
                continue
            nxt = mods[i + 3] if i + 3 < len(mods) and is_conv(mods[i + 3]) else None
            hand = False
            if self.codes and nxt is not None and hasattr(mod, "codes_ready") and hasattr(nxt, "codes_ready"):
                probe = torch.empty(1, dtype=torch.uint8, device=y.device).expand(_out_shape(mod, y.shape))
                hand = mod.codes_ready(y)[1] and nxt.codes_ready(probe)[0]
            if hand:
                scale, shift = self.tables(bn)
                y = mod.forward_fused(y, scale, shift, relu=True, out_quant=nxt, keep_float=False)
                self.code_edges.append((names[id(mod)], names[id(nxt)], "codes"))
            else:
                if y.dtype == torch.uint8 and not (hasattr(mod, "fused_epilogue_ready") and mod.fused_epilogue_ready(y)):
                    raise RuntimeError("FusedEval: a conv stopped taking the library path during a forward")
                y = self._conv(mod, bn, y)
            i += 3
        return self.model.classifier(y.flatten(1))

    def forward(self, x):
        if torch.is_grad_enabled():
            raise RuntimeError("FusedEval is evaluation only: call it under torch.no_grad()")
        if isinstance(self.model, VGG):
            if self.net and self.pool:  # the max-pools in the convs' kernels: the whole network is one plan
                y = self._forward_net(x)
                self.net_used = y is not None
                if y is not None:
                    return y
            elif self.net:
                self.net_used = False
                self.net_reason = "a VGG runs in the loop: its max-pools are torch operations (pool=True moves them " \
                                  "into the convs' kernels)"
            return self._forward_vgg(x)
        if self.net:
            y = self._forward_net(x)
            self.net_used = y is not None
            if y is not None:
                return y
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
