"""LSQ and CiM quantised modules -- MI355X drop-in for models/_modules/lsq.py.

``Conv2dLSQCiM`` keeps the reference's constructor, parameters, buffers, first-step
initialisation and output layout, and runs the quantised conv on libcimq's HIP kernels:
the activation quantiser is fused into the CiM kernels (x_q is never materialised), the
partial sums are integer MFMA products, the ADC is applied from exact integer thresholds.
``get_cim_output_signed`` is re-exported with the reference's 17-argument signature.

``Conv2dLSQ`` / ``LinearLSQ`` / ``ActLSQ`` (plain LSQ fake-quant, unused by the CiM
example, SURVEY.md section 8f "next") run their quantisers on libcimq and Conv2dLSQ's conv of
integer codes on int8 MFMA (functional.lsq_quantize / qconv2d).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from ..functional import (alpha_cim_init, cim_conv2d_lsq, cim_conv2d_lsq_shift, cim_module_conv,  # noqa: F401
                          act_codes_of, cim_module_conv_codes, cim_module_conv_epilogue, cim_module_conv_pool,
                          cim_module_shift_conv, get_adcless_cim_output, get_analog_partial_sums_autograd_ver2,
                          conv_out_hw, get_cim_output_signed, inference_call, inference_weights, lsq_quantize,
                          module_descs, module_shift_supported, qconv2d)
from ._quan_base import (_ActQ, _Conv2dQ, _Conv2dQCiM, _LinearQ, Qmodes, grad_scale,  # noqa: F401
                         round_pass)

__all__ = ["Conv2dLSQ", "LinearLSQ", "ActLSQ", "Conv2dLSQCiM"]


def _act_range(nbits):
    return 0, 2 ** nbits - 1


def _weight_range(nbits):
    return -(2 ** (nbits - 1)), 2 ** (nbits - 1) - 1


def _adc_qp(adcbits):
    if adcbits in (1, 1.5):
        return 1
    return 2 ** (adcbits - 1) - 1


class Conv2dLSQCiM(_Conv2dQCiM):
    """CiM-aware LSQ conv (lsq.py:511-588) on MI355X.

    ``adc_shift=True`` (this build's option, off by default so the state_dict matches the
    reference): a learnable per-(tile, w-slice, a-slice, channel) shift ``beta_cim`` next to
    ``alpha_cim``, and the ADC of test/test_backward_cimlayer_scale_shift.py on the rescaled
    partial sum u -- adcbits 1.5: clamp(round((u-beta)/alpha_q), -1, 1)*alpha_q + beta (ver2);
    adcbits 1: sign((u-beta)/alpha_q)*alpha_q + beta (adcless).  beta starts at 0.

    Evaluation: a forward under ``torch.no_grad()`` (or one no input of which requires a gradient) runs
    the library's forward-only mode -- the same output bit for bit, no backward state, nothing saved.
    On the fused library-ADC path, and on the fused shift path (beta_cim then counts among the parameters), the
    layer then keeps the weight side it prepared (``_inf_prep``) and
    reuses it while the input shape and the parameters' versions and addresses are unchanged, so a whole
    evaluation quantises the weights once per input shape.  ``train(True)`` and ``load_state_dict`` drop
    it, a call made with grad enabled never reads it, and stochastic-ADC layers keep none.  An edit
    through ``p.data`` bumps no version counter (functional._versions): after one, call ``train()`` /
    ``eval()`` again or torch.autograd.graph.increment_version(p) before the next evaluation."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1,
                 groups=1, bias=True, nbits_w=8, nbits_a=8, nbits_alpha=8, wbitslice=1, abitslice=1,
                 xbar=64, adcbits=6, stochastic_quant=False, adc_shift=False, **kwargs):
        super().__init__(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size,
                         stride=stride, padding=padding, dilation=dilation, groups=groups, bias=bias,
                         nbits_w=nbits_w, nbits_a=nbits_a, nbits_alpha=nbits_alpha, wbitslice=wbitslice,
                         abitslice=abitslice, xbar=xbar, adcbits=adcbits, stochastic_quant=stochastic_quant)
        self.adc_shift = bool(adc_shift)
        if self.adc_shift:
            if adcbits not in (1, 1.5) or stochastic_quant:
                raise ValueError("adc_shift needs a deterministic 1- or 1.5-bit ADC (adcbits 1 / 1.5)")
            self.beta_cim = torch.nn.Parameter(torch.zeros_like(self.alpha_cim))
        else:
            self.beta_cim = None
        self._state_cache = None  # host mirror of (init_state, init_state_cim) to avoid a sync per step
        self.fused = True  # steady state through cimq_module_forward/backward (False: torch quantisers)
        # parameter grads added into the existing .grad buffers inside the library (no
        # AccumulateGrad kernels); set by dist.GradBucket.own(), which owns the exchange
        self.accumulate_grads_in_place = False
        self.tail_stream = None  # GradBucket.own(overlap=True): stream of the parameter-gradient epilogue
        # CIMQ_OPT_RECOMPUTE: where the library has a recompute backward for this shape, keep no per-partial-sum
        # state words between forward and backward (33.5 MB less per 16-channel ResNet-20 layer at B = 256) and
        # recompute the partial sums in the backward -- slower on MI355X, so off by default
        self.recompute_psum = False
        self._wprep = None        # functional.prepare_weights: the next forward's weight side, computed ahead
        self._inf_prep = None     # functional.inference_weights: the weight side the no-grad forwards share
        self._last_x_shape = None

    def layer_config(self):
        """(stride, padding, dilation, nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar, nbits_alpha): the
        configuration the functional entry points take positionally, as the attributes are now."""
        return (self.stride, self.padding, self.dilation, self.nbits_a, self.abitslice, self.nbits_w, self.wbitslice,
                self.adcbits, self.xbar, self.nbits_alpha)

    def _out_hw(self, x_shape):
        return conv_out_hw(x_shape[-2], x_shape[-1], *self.weight.shape[-2:], self.stride, self.padding)

    def _fused_ready(self):
        """True once the steady-state library path applies and an input shape is known
        (prepare_weights needs both)."""
        flags = self._init_flags()
        return (self.fused and flags[0] and (flags[1] or self.alpha_cim is None) and self.adcbits != 0
                and not self.adc_shift and not self.stochastic_quant and self._last_x_shape is not None
                and self.weight.is_cuda)

    def _shift_fused(self, x):
        """Whether libcimq's fused shift path takes input shape x.shape (cached per shape)."""
        key = tuple(x.shape)
        if getattr(self, "_shift_ok", None) is None or self._shift_ok[0] != key:
            self._shift_ok = (key, x.is_cuda and module_shift_supported(key, self.weight, *self.layer_config()))
        return self._shift_ok[1]

    def _load_from_state_dict(self, *args, **kwargs):
        self._state_cache = None
        self._inf_prep = None
        return super()._load_from_state_dict(*args, **kwargs)

    def train(self, mode=True):
        if mode:
            self._inf_prep = None
        return super().train(mode)

    def _init_flags(self):
        key = (self.init_state._version, self.init_state_cim._version)
        if self._state_cache is None or getattr(self, "_state_key", None) != key:
            self._state_cache = [bool(self.init_state.item() != 0), bool(self.init_state_cim.item() != 0)]
            self._state_key = key
        return self._state_cache

    def forward(self, x):
        qn_w, qp_w = _weight_range(self.nbits_w)
        qp_adc = _adc_qp(self.adcbits)
        qn_a, qp_a = _act_range(self.nbits_a)
        flags = self._init_flags()
        if self.training and not flags[0]:
            # lsq.py:532-542: sign detection and LSQ step-size init on the first training step
            if x.min() < -1e-5:
                self.signed_act.data.fill_(1)
            self.alpha_act.data.copy_(2 * x.abs().mean() / math.sqrt(qp_a))
            self.alpha_weight.data.copy_(2 * self.weight.abs().mean() / math.sqrt(qp_w))
            self.init_state.fill_(1)
            flags[0] = True
        if self.binary_mask.device != x.device:
            self.binary_mask = self.binary_mask.to(x.device)
        if (self.fused and self.adc_shift and flags[0] and flags[1] and self._shift_fused(x)):
            # steady state of the shift ADC on libcimq's fused path (quantisers in the library)
            wprep = None
            if (not torch.is_grad_enabled() and x.is_cuda and
                    inference_call(x, self.weight, self.alpha_act, self.alpha_weight, self.alpha_cim, self.beta_cim)):
                # evaluation: the forward-only weight side (beta_cim in it), made once and kept while it matches
                wprep = self._inf_prep = inference_weights(self, x.shape, self._inf_prep)
            cfg = self.layer_config()
            out = cim_module_shift_conv(x, self.weight, self.alpha_act, self.alpha_weight, self.alpha_cim,
                                        self.beta_cim, self.binary_mask, self.signed_act, *cfg[:7], *cfg[8:],
                                        wprep=wprep)  # (no adcbits: the fused shift path is 1.5-bit)
            return out if self.bias is None else out + self.bias  # lsq.py:583's broadcast
        if (self.fused and flags[0] and (flags[1] or self.alpha_cim is None) and self.adcbits != 0
                and not self.adc_shift):
            # steady state: the three quantisers and the CiM conv in one library call each way (the
            # weight side possibly prepared ahead by prepare_weights; taken once)
            wprep, self._wprep = self._wprep, None
            self._last_x_shape = tuple(x.shape)
            if (not torch.is_grad_enabled() and not self.stochastic_quant and x.is_cuda and
                    inference_call(x, self.weight, self.alpha_act, self.alpha_weight, self.alpha_cim)):
                # evaluation: the forward-only weight side, made once and kept while it matches
                wprep = self._inf_prep = inference_weights(self, x.shape, self._inf_prep)
            out = cim_module_conv(x, self.weight, self.alpha_act, self.alpha_weight, self.alpha_cim,
                                  self.binary_mask, self.signed_act, *self.layer_config(),
                                  self.accumulate_grads_in_place, bool(self.stochastic_quant),
                                  self.tail_stream if self.accumulate_grads_in_place else None, wprep,
                                  self.recompute_psum)
            if self.bias is not None:
                out = out + self.bias  # broadcasts over the last axis, as lsq.py:583
            return out
        sa = grad_scale(self.alpha_act, 1.0 / math.sqrt(x.numel() * qp_a))            # lsq.py:547-548
        sw = grad_scale(self.alpha_weight, 1.0 / math.sqrt(self.weight.numel() * qp_w))  # lsq.py:553-554
        w_q = round_pass((self.weight / sw).clamp(qn_w, qp_w)) * sw                   # lsq.py:555
        if self.training and not flags[1] and self.alpha_cim is not None:
            with torch.no_grad():                                                      # lsq.py:557-563
                a0 = alpha_cim_init(x, w_q, sa, sw, self.binary_mask, self.signed_act, self.stride,
                                    self.padding, self.nbits_a, self.abitslice, self.nbits_w,
                                    self.wbitslice, self.adcbits, self.xbar, self.num_xbars)
                self.alpha_cim.data.copy_(a0)
                self.init_state_cim.fill_(1)
            flags[1] = True
        alpha_q = None
        if self.alpha_cim is not None:                                                 # lsq.py:566-571
            qp_al, qn_al = 2 ** self.nbits_alpha - 1, 1
            a = self.alpha_cim
            scale = (a.max() - a.min()) / (qp_al - qn_al)
            alpha_q = round_pass(a / scale).clamp(qn_al, qp_al) * scale
        if self.adcbits == 0:                                                          # lsq.py:584-585
            x_q = round_pass((x / sa).clamp(qn_a, qp_a)) * sa
            return F.conv2d(x_q, w_q, self.bias, self.stride, self.padding, self.dilation)
        cfg = self.layer_config()[:9]  # (these two take no nbits_alpha: alpha_q is quantised above)
        if self.adc_shift:
            out = cim_conv2d_lsq_shift(x, w_q, sa, sw, alpha_q, self.beta_cim, self.binary_mask, self.signed_act, *cfg)
        else:
            out = cim_conv2d_lsq(x, w_q, sa, sw, alpha_q, self.binary_mask, self.signed_act, *cfg,
                                 bool(self.stochastic_quant))
        # lsq.py:123's fold_x, per axis (the same number twice for the reference's square layers)
        out = out.transpose(1, 2).view(x.shape[0], self.out_channels, *self._out_hw(x.shape))  # lsq.py:580-581
        if self.bias is not None:
            out = out + self.bias  # broadcasts over the last axis, as lsq.py:583
        return out

    def fused_epilogue_ready(self, x):
        """Whether ``forward_fused`` takes this layer for input ``x``: the steady-state library path (both
        first-step initialisations done, a CiM ADC, ROCm tensors; the shift ADC where libcimq fuses it) and no
        bias -- the reference's bias broadcasts over the last axis (lsq.py:583), so it is no per-channel term."""
        flags = self._init_flags()
        if not (self.fused and flags[0] and (flags[1] or self.alpha_cim is None) and self.adcbits != 0
                and self.bias is None and torch.is_tensor(x) and x.is_cuda and self.weight.is_cuda):
            return False
        return self._shift_fused(x) if self.adc_shift else True

    def _code_quant(self, numel):
        """(alpha_act, gscale_a, Qp) of this layer's activation quantiser for an input of ``numel`` elements: what
        a producer needs to write this layer's codes (cim_module_conv_codes' ``out_quant``)."""
        qp_a = float(_act_range(self.nbits_a)[1])
        return self.alpha_act, 1.0 / math.sqrt(numel * qp_a), qp_a

    def act_codes(self, y):
        """The activation codes of an fp32 tensor ``y`` entering this layer, in torch (the twin of the codes
        libcimq writes and reads, include/cimq.h cimq_act_codes): ``rint(clamp(y / sa, 0, Qp))`` as uint8 with
        sa the step size ``forward`` computes for an input of y's size, and Qp + 1 where y is NaN.  Computed on
        y's device; move y to the host first where the division must be IEEE."""
        return act_codes_of(y, *self._code_quant(y.numel()))

    def _codes_desc(self, shape):
        key = tuple(shape)
        hit = getattr(self, "_codes_ok", None)
        if hit is None or hit[0] != key:
            from .. import _lib
            # (a query of the route alone: module_descs never builds the stochastic form, which would draw a seed)
            desc, _ = module_descs(self, key, inference=True)
            hit = self._codes_ok = (key, _lib.codes_supported(desc))
        return hit[1]

    def codes_ready(self, x):
        """``(in_ok, out_ok)``: whether ``forward_fused`` takes this layer's input ``x`` as codes (a
        ``torch.uint8`` x), and whether it can write its output as codes (``out_quant``) -- ``fused_epilogue_ready``
        and what cimq_module_codes_supported answers for x's shape (cached per shape).  ``x``: the input as fp32
        or as codes; only its shape and device matter."""
        if not self.fused_epilogue_ready(x):
            return False, False
        return self._codes_desc(x.shape)

    def pool_ready(self, x):
        """Whether ``forward_fused(..., pool=2)`` takes this layer for input ``x``: ``fused_epilogue_ready``, a
        library-ADC layer, and what cimq_module_pool_supported answers for x's shape (cached per shape): the wide
        forward route with an output at most 32 wide.  Only x's shape and device matter."""
        if not self.fused_epilogue_ready(x) or self.adc_shift or self.stochastic_quant:
            return False
        key = tuple(x.shape)
        hit = getattr(self, "_pool_ok", None)
        if hit is None or hit[0] != key:
            from .. import _lib
            desc, _ = module_descs(self, key, inference=True)
            hit = self._pool_ok = (key, _lib.module_pool_supported(desc))
        return hit[1]

    def forward_fused(self, x, scale, shift, residual=None, relu=False, *, out_quant=None, keep_float=True, pool=None):
        """Evaluation only: ``forward(x)`` with a per-channel affine (a folded BatchNorm: ``scale``, ``shift``,
        [out_channels] fp32), an optional ``residual`` (the output's shape; made contiguous fp32 if it is not) and an
        optional ReLU applied in the forward kernel's registers before the store -- bit for bit
        ``relu(forward(x) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) + residual)`` in that order of
        operations (cim_module_conv_epilogue).  Uses the kept inference weight side exactly as ``forward`` does.
        Raises where ``fused_epilogue_ready`` does not hold, or if the call could be differentiated.
        Activation codes (cim_module_conv_codes; without them the call is the one above, unchanged): a
        ``torch.uint8`` ``x`` is this layer's input as codes (``act_codes``), and the output is bit for bit that of
        any fp32 input with those codes; ``out_quant=next_conv`` also returns the output's codes for that layer,
        written by the kernel that stores the output -- ``(output, codes)``, or with ``keep_float=False`` the codes
        alone.  ``codes_ready`` says which of the two this layer supports.
        ``pool=2``: the storing kernel writes the 2x2 / stride-2 max pool of those values instead
        (cim_module_conv_pool): [B, O, Ho/2, Wo/2], bit for bit ``F.max_pool2d(forward_fused(...), 2, 2)``; the
        residual keeps the unpooled shape.  Raises where ``pool_ready`` does not hold, and with codes on either side."""
        if pool is not None and pool != 2:
            raise ValueError("Conv2dLSQCiM.forward_fused: pool must be None or 2")
        if pool and (out_quant is not None or torch.is_tensor(x) and x.dtype == torch.uint8):
            raise ValueError("Conv2dLSQCiM.forward_fused: pool takes fp32 in and writes fp32 out (no out_quant, no codes)")
        if pool and not self.pool_ready(x):
            raise RuntimeError("Conv2dLSQCiM.forward_fused(pool=2) needs the steady-state library path, the library "
                               "ADC and a layer on the wide forward route at most 32 output columns wide (pool_ready)")
        if not self.fused_epilogue_ready(x):
            raise RuntimeError("Conv2dLSQCiM.forward_fused needs the steady-state library path (both first-step "
                               "initialisations done, adcbits != 0, ROCm tensors) and bias=None")
        if self.binary_mask.device != x.device:
            self.binary_mask = self.binary_mask.to(x.device)
        wprep = None
        if not self.adc_shift:
            self._last_x_shape = tuple(x.shape)
        if not torch.is_grad_enabled() and not self.stochastic_quant:
            wprep = self._inf_prep = inference_weights(self, x.shape, self._inf_prep)
        if x.dtype != torch.uint8 and out_quant is None:
            if not keep_float:
                raise ValueError("Conv2dLSQCiM.forward_fused: keep_float=False needs out_quant")
            if pool:
                return cim_module_conv_pool(
                    x, self.weight, self.alpha_act, self.alpha_weight, self.alpha_cim, self.binary_mask,
                    self.signed_act, *self.layer_config(), scale, shift, residual=residual, relu=relu, pool=pool,
                    wprep=wprep, recompute=self.recompute_psum)
            return cim_module_conv_epilogue(
                x, self.weight, self.alpha_act, self.alpha_weight, self.alpha_cim, self.binary_mask, self.signed_act,
                *self.layer_config(), scale, shift, residual=residual, relu=relu,
                beta_cim=self.beta_cim if self.adc_shift else None, stochastic=bool(self.stochastic_quant),
                wprep=wprep, recompute=self.recompute_psum)
        oq = None
        if out_quant is not None:
            ho, wo = self._out_hw(x.shape)
            oq = out_quant._code_quant(x.shape[0] * self.out_channels * ho * wo)
        return cim_module_conv_codes(
            x, self.weight, self.alpha_act, self.alpha_weight, self.alpha_cim, self.binary_mask, self.signed_act,
            *self.layer_config(), scale, shift, residual=residual, relu=relu,
            beta_cim=self.beta_cim if self.adc_shift else None, stochastic=bool(self.stochastic_quant), wprep=wprep,
            recompute=self.recompute_psum, out_quant=oq, keep_float=keep_float)


class _HostFlags:
    """Host mirror of the init_state (and ActLSQ's signed) buffers for the plain modules.

    The reference tests ``self.init_state == 0`` (and ActLSQ ``self.signed == 1``) on every
    forward (lsq.py:407, :601, :628, :634, :643); on a GPU tensor each test is a device sync that stalls the
    launch queue. The values are read once and cached, keyed by the buffers' version counters: any
    in-place write to them -- load_state_dict, dist.GradBucket.broadcast_from, torch DDP's buffer
    broadcast from rank 0 before every forward (train.py:232 wraps the model in DDP) -- bumps the counter
    and the next forward re-reads them, so a rank follows rank 0's buffers as the reference does.  Writes
    through ``.data`` (which bypass the counter) update the cache alongside.

    Cost under torch DDP with ``broadcast_buffers=True`` (its default): the per-forward buffer broadcast
    bumps the counters on every step, so every module re-reads its flags with a blocking ``.item()`` per
    forward -- the device sync this cache exists to avoid.  The buffers only change in the first
    (initialising) step, so prefer ``dist.GradBucket`` (one exchange per step, broadcast_from(0) after the
    first step) or DDP with ``broadcast_buffers=False`` after that step."""

    _state_cache = None
    _state_key = None

    def _load_from_state_dict(self, *args, **kwargs):
        self._state_cache = None
        return super()._load_from_state_dict(*args, **kwargs)

    def _flags(self):
        sg = getattr(self, "signed", None)
        key = (self.init_state._version, -1 if sg is None else sg._version)
        if self._state_cache is None or self._state_key != key:
            self._state_cache = [bool(self.init_state.item() != 0), sg is not None and bool(sg.item() == 1)]
            self._state_key = key
        return self._state_cache


class Conv2dLSQ(_HostFlags, _Conv2dQ):
    """Plain LSQ conv (lsq.py:389-436); consumes the (x_q, act_scale) tuple of ActLSQ.

    The weight quantiser runs on libcimq (lsq_quantize) and the conv of the two integer-code
    tensors on int8 MFMA (qconv2d) when x_q comes from this package's ActLSQ (codes by
    construction, their range recorded on the tensor); any other x_q -- the reference accepts
    arbitrary tensors in the tuple -- is convolved by torch's fp32 conv."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1,
                 groups=1, bias=True, nbits_w=8, **kwargs):
        super().__init__(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size,
                         stride=stride, padding=padding, dilation=dilation, groups=groups, bias=bias,
                         nbits=nbits_w)

    def forward(self, x):
        if self.alpha is None:
            return F.conv2d(x, self.weight, self.bias, self.stride, self.padding, self.dilation, self.groups)
        x_q, act_scale = x
        qn, qp = _weight_range(self.nbits)
        if self.training and not self._flags()[0]:
            self.alpha.data.copy_(2 * self.weight.abs().mean() / math.sqrt(qp))
            self.init_state.fill_(1)
            self._flags()[0] = True
        ws = grad_scale(self.alpha, 1.0 / math.sqrt(self.weight.numel() * qp))
        w_q = lsq_quantize(self.weight, ws, qn, qp)
        code_range = getattr(x_q, "_cimq_code_range", None)
        if code_range is not None and self.groups == 1 and self.nbits <= 8:
            return qconv2d(x_q, act_scale, w_q, ws, self.bias, self.stride, self.padding, self.dilation,
                           code_range)
        y = F.conv2d(x_q, w_q, self.bias, self.stride, self.padding, self.dilation, self.groups)
        return y * act_scale * ws


class LinearLSQ(_HostFlags, _LinearQ):
    """Plain LSQ linear (lsq.py:591-617): the weight quantiser on libcimq, the fp32 linear of the
    unquantised input by torch's GEMM (the reference quantises only the weight here)."""

    def __init__(self, in_features, out_features, bias=True, nbits_w=4, **kwargs):
        super().__init__(in_features=in_features, out_features=out_features, bias=bias, nbits=nbits_w)

    def forward(self, x):
        if self.alpha is None:
            return F.linear(x, self.weight, self.bias)
        qn, qp = _weight_range(self.nbits)
        if self.training and not self._flags()[0]:
            self.alpha.data.copy_(2 * self.weight.abs().mean() / math.sqrt(qp))
            self.init_state.fill_(1)
            self._flags()[0] = True
        a = grad_scale(self.alpha, 1.0 / math.sqrt(self.weight.numel() * qp))
        return F.linear(x, lsq_quantize(self.weight, a, qn, qp, scaled=True), self.bias)


class ActLSQ(_HostFlags, _ActQ):
    """LSQ activation quantiser (lsq.py:620-662): returns (integer codes, step size); the codes
    come from libcimq and carry their range for Conv2dLSQ's int8 conv."""

    def __init__(self, nbits_a=4, **kwargs):
        super().__init__(nbits=nbits_a)

    def _range(self):
        if self._flags()[1]:
            return -(2 ** (self.nbits - 1)), 2 ** (self.nbits - 1) - 1
        return 0, 2 ** self.nbits - 1

    def forward(self, x):
        if self.alpha is None:
            return x
        if self.training and not self._flags()[0]:
            if x.min() < -1e-5:
                self.signed.data.fill_(1)
                self._flags()[1] = True
            _, qp = self._range()
            self.alpha.data.copy_(2 * x.abs().mean() / math.sqrt(qp))
            self.init_state.fill_(1)
            self._flags()[0] = True
        qn, qp = self._range()
        a = grad_scale(self.alpha, 1.0 / math.sqrt(x.numel() * qp))
        x_q = lsq_quantize(x, a, qn, qp)
        if -128 <= qn and qp <= 255 and (qn >= 0 or qp <= 127):
            x_q._cimq_code_range = (int(qn), int(qp))
        return x_q, a
