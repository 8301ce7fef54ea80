"""Autograd Functions backed by libcimq (HIP, gfx950).

``get_cim_output_signed``  drop-in for the reference Function of the same name
                           (models/_modules/lsq.py:89-386): same 17 positional args,
                           same [B, P, O] output, same 17-tuple of grads.
``cim_conv2d_lsq``         the fused path used by ``Conv2dLSQCiM``: the activation LSQ
                           quantiser (lsq.py:547-549) runs inside the CiM kernels, so x_q
                           is never materialised; grads flow to x and to the step size sa.
``get_analog_partial_sums_autograd_ver2`` / ``get_adcless_cim_output``
                           drop-ins for the scale + shift ADC Functions of
                           test/test_backward_cimlayer_scale_shift.py (:336-546 / :113-334):
                           same 14 positional args, grads for x, w, alpha_cim, beta_cim.
``cim_conv2d_lsq_shift``   the scale + shift ADC as a Conv2dLSQCiM option (adc_shift=True).

Inference: a call made under ``torch.no_grad()`` / ``torch.inference_mode()``, or with no tensor
argument that requires a gradient, runs the library's forward-only mode (CIMQ_OPT_INFERENCE, ABI 15):
the same ``out`` bit for bit, no backward state written, a ctx of the weight tables only, nothing
saved.  The choice is made before ``Function.apply`` (inside ``forward`` grad mode is always off and
``needs_input_grad`` is all True, whatever the caller's mode).

One marshalling path: every conv call takes its sizes from ``_geometry``, its tensors from ``_operands`` (an
``Operands``, which is also every Function's ``ctx.bufs``) and, at the module entry points, its descriptors,
prepared weight side and buffers from ``_layer_call``; a backward places its gradients with ``_grads``.

Device-only: CPU tensors raise (there is no CPU fallback in the product path).
"""
from __future__ import annotations

import contextlib
import ctypes
import inspect
import math

import torch

from . import _lib


_INFERENCE = True  # tests switch it off to compare against the training forward under no-grad


def inference_call(*args) -> bool:
    """Whether a call with these arguments can never be differentiated: grad mode is off, or no
    tensor among them requires a gradient.  Such calls take the forward-only library path."""
    if not _INFERENCE:
        return False
    if not torch.is_grad_enabled():
        return True
    return not any(torch.is_tensor(a) and a.requires_grad for a in args)


def _require_device(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("cim_quantization_amd runs on ROCm devices only (got a CPU tensor); "
                               "the CPU restatement lives in oracle/ and is test infrastructure")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def stochastic_seed() -> int:
    """Philox key of one stochastic-ADC call, drawn from torch's default CPU generator: the
    draws are reproducible under ``torch.manual_seed`` (the reference draws torch.cuda
    uniform_ noise, lsq.py:215-216) and no device synchronisation is needed."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def _dense(t, device, dtype):
    """``t`` detached, contiguous, of ``dtype`` on ``device``.  A tensor that already is all that comes back as a
    view of its own storage (what ``.to().contiguous()`` gives too, without their dispatch cost on every call)."""
    if not isinstance(t, torch.Tensor):
        t = torch.tensor(t)
    if t.dtype is dtype and t.device == device and t.is_contiguous():
        return t.detach()
    return t.detach().to(device=device, dtype=dtype).contiguous()


def _f32(t, device):
    return _dense(t, device, torch.float32)


def _one(t, device):
    """A scalar argument (a step size, signed_act) as the fp32 tensor whose first element the library reads."""
    t = _dense(t, device, torch.float32)
    return t if t.numel() == 1 else t.reshape(-1)[:1].contiguous()


def _ptrs(*ts):
    """The device addresses of consecutive library arguments (None for an absent one)."""
    return [None if t is None else t.data_ptr() for t in ts]


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _ubuf(nbytes, device):
    return torch.empty(max(nbytes, 1), device=device, dtype=torch.uint8)


def conv_out_hw(H, W, KH, KW, stride, padding):
    """Output height and width of the CiM conv (dilation 1; lsq.py:123's fold_x, per axis)."""
    return (H + 2 * padding[0] - KH) // stride[0] + 1, (W + 2 * padding[1] - KW) // stride[1] + 1


def out_hw(desc):
    """conv_out_hw of a ``_lib.ConvDesc``."""
    return conv_out_hw(desc.in_h, desc.in_w, desc.kernel_h, desc.kernel_w, (desc.stride_h, desc.stride_w),
                       (desc.pad_h, desc.pad_w))


def _geometry(x, w, stride, padding, dilation):
    """(B, C, H, W, O, KH, KW, stride pair, padding pair, Ho, Wo) of one conv call."""
    stride, padding = _pair(stride), _pair(padding)
    if _pair(dilation) != (1, 1):
        # lsq.py:141 unfolds without dilation while lsq.py:382 folds with it; only 1 is consistent
        raise NotImplementedError("CiM conv supports dilation 1 only (as the reference's unfold)")
    B, C, H, W = x.shape
    O, Cw, KH, KW = w.shape
    if Cw != C:
        raise ValueError(f"weight in_channels {Cw} != input channels {C} (groups are not supported)")
    return (B, C, H, W, O, KH, KW, stride, padding) + conv_out_hw(H, W, KH, KW, stride, padding)


class Operands:
    """The tensors of one conv call as the library reads them, by name; every Function's ``ctx.bufs``.
    ``sa`` / ``sw``: the activation / weight step sizes (the module entry points' alpha_act / alpha_weight);
    ``alpha`` / ``beta``: alpha_cim / beta_cim, or None; ``ctx``: the call's ctx buffer (uint8)."""

    __slots__ = ("x", "w", "sa", "sw", "alpha", "beta", "mask", "sgn", "ctx")


def _operands(x, w, sa, sw, alpha, beta, mask, sgn, x_codes=False):
    """Operands of a call on ``x``'s device: contiguous fp32 tensors, [1] scalars, an int8 mask; ``ctx`` is left
    to the caller.  A contiguous fp32 tensor already there passes through as a view of its own storage, so the
    library reads a parameter where it lives (_versions and the one-call plan rely on that).  ``x_codes``: x
    holds uint8 activation codes, taken as they are."""
    dev, f32 = x.device, torch.float32
    o = Operands()
    o.x = x.detach().contiguous() if x_codes else _dense(x, dev, f32)
    o.w = _dense(w, dev, f32)
    o.sa, o.sw = _one(sa, dev), _one(sw, dev)
    o.alpha = None if alpha is None else _dense(alpha, dev, f32)
    o.beta = None if beta is None else _dense(beta, dev, f32)
    o.mask = _dense(mask, dev, torch.int8)
    o.sgn = _one(sgn, dev)
    o.ctx = None
    return o


def _arg_names(forward):
    """The argument names of a Function's ``forward`` after ctx: its backward returns one gradient for each."""
    return tuple(inspect.signature(forward).parameters)[1:]


def _grads(names, **by_name):
    """A backward's result: the given gradients at their arguments' positions among ``names``, None elsewhere
    (a name the forward does not have raises)."""
    out = [None] * len(names)
    for k, g in by_name.items():
        out[names.index(k)] = g
    return tuple(out)


def _cim_forward(x, w, sa, sw, alpha, binary_mask, signed_act, stride, padding, dilation, act_bits, act_bs, w_bits,
                 w_bs, adc_bits, arr, stochastic, input_kind, qp_a, inference=False):
    """cimq_forward on quantised values (CIMQ_INPUT_XQ) or on the raw activation (CIMQ_INPUT_RAW_LSQ, clamp
    maximum ``qp_a``); returns (out, desc, sizes, operands).  ``inference``: CIMQ_OPT_INFERENCE."""
    _require_device(x)
    B, C, H, W, O, KH, KW, st, pd, Ho, Wo = _geometry(x, w, stride, padding, dilation)
    desc = _lib.make_desc(B, C, H, W, O, KH, KW, st, pd, arr, w_bits, act_bits, w_bs, act_bs, adc_bits, input_kind,
                          qp_a, _lib.CIMQ_ADC_STOCHASTIC if stochastic else _lib.CIMQ_ADC_LIBRARY,
                          stochastic_seed() if stochastic else 0, _lib.CIMQ_OPT_INFERENCE if inference else 0)
    sizes = _lib.query_sizes(desc)
    o = _operands(x, w, sa, sw, alpha, None, binary_mask, signed_act)
    out = torch.empty(B, Ho * Wo, O, device=x.device, dtype=torch.float32)
    o.ctx = _ubuf(sizes.ctx_bytes, x.device)
    _lib.check(_lib.load().cimq_forward(desc, *_ptrs(o.x, o.w, o.sa, o.sw, o.alpha, o.mask, o.sgn, out, o.ctx), None,
                                        _stream()), "cimq_forward")
    return out, desc, sizes, o


def _cim_backward(ctx, grad_output, want_gsa):
    """cimq_backward of a _cim_forward ctx; returns (grad_x, grad_w, grad_alpha or None, grad_sa or None)."""
    ctx.saved_tensors  # noqa: B018 -- raises if x / w changed in place since the forward
    o = ctx.bufs
    dev = o.x.device
    g = _f32(grad_output, dev)
    gx = torch.empty_like(o.x)
    gw = torch.empty_like(o.w)
    gsa = torch.empty(1, device=dev, dtype=torch.float32) if want_gsa else None
    ga = None if o.alpha is None else torch.empty_like(o.alpha)
    ws = _ubuf(ctx.sizes.bwd_workspace_bytes, dev)
    _lib.check(_lib.load().cimq_backward(ctx.desc, *_ptrs(g, o.x, o.sa, o.sw, o.alpha, o.mask, o.sgn, o.ctx, gx, gw,
                                                          ga, gsa, ws), _stream()), "cimq_backward")
    return gx, gw, ga, gsa


class get_cim_output_signed(torch.autograd.Function):
    """HIP implementation of ``get_cim_output_signed`` (lsq.py:89-386)."""

    @classmethod
    def apply(cls, *args):
        """The Function, or for a call nothing can differentiate (inference_call) the forward-only
        library call: same output, no autograd node, no saved state."""
        if inference_call(*args):
            return cls._call(*args, inference=True)[0]
        return super().apply(*args)

    @staticmethod
    def _call(x, w, conv_stride, conv_padding, conv_dilation, act_bits, act_bit_slice,
              weight_bits, weight_bit_slice, adc_bits, arr, binary_mask, alpha_cim,
              weight_scaling_factor, act_scaling_factor, stochastic, signed_act, inference=False):
        if stochastic:
            assert adc_bits == 1.5  # lsq.py:136-137
        return _cim_forward(x, w, act_scaling_factor, weight_scaling_factor, alpha_cim, binary_mask, signed_act,
                            conv_stride, conv_padding, conv_dilation, act_bits, act_bit_slice, weight_bits,
                            weight_bit_slice, adc_bits, arr, stochastic, _lib.CIMQ_INPUT_XQ, 0.0, inference)

    @staticmethod
    def forward(ctx, x, w, conv_stride, conv_padding, conv_dilation, act_bits, act_bit_slice,
                weight_bits, weight_bit_slice, adc_bits, arr, binary_mask, alpha_cim,
                weight_scaling_factor, act_scaling_factor, stochastic, signed_act):
        out, ctx.desc, ctx.sizes, ctx.bufs = get_cim_output_signed._call(
            x, w, conv_stride, conv_padding, conv_dilation, act_bits, act_bit_slice, weight_bits, weight_bit_slice,
            adc_bits, arr, binary_mask, alpha_cim, weight_scaling_factor, act_scaling_factor, stochastic, signed_act)
        ctx.save_for_backward(x, w)  # autograd's version check: in-place edits before backward raise
        return out

    _ARGS = _arg_names(forward.__func__)

    @staticmethod
    def backward(ctx, grad_output):
        gx, gw, ga, _ = _cim_backward(ctx, grad_output, False)
        return _grads(get_cim_output_signed._ARGS, x=gx, w=gw, alpha_cim=ga)


class _CimConv2dLSQ(torch.autograd.Function):
    """Fused LSQ-activation-quantiser + CiM conv (lsq.py:547-549 followed by lsq.py:578)."""

    @staticmethod
    def _call(x, w_q, sa, sw, alpha_q, binary_mask, signed_act, stride, padding, dilation,
              nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar, stochastic=False, inference=False):
        return _cim_forward(x, w_q, sa, sw, alpha_q, binary_mask, signed_act, stride, padding, dilation, nbits_a,
                            abitslice, nbits_w, wbitslice, adcbits, xbar, stochastic, _lib.CIMQ_INPUT_RAW_LSQ,
                            float(2 ** nbits_a - 1), inference)

    @staticmethod
    def forward(ctx, x, w_q, sa, sw, alpha_q, binary_mask, signed_act, stride, padding, dilation,
                nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar, stochastic=False):
        out, ctx.desc, ctx.sizes, ctx.bufs = _CimConv2dLSQ._call(
            x, w_q, sa, sw, alpha_q, binary_mask, signed_act, stride, padding, dilation, nbits_a, abitslice, nbits_w,
            wbitslice, adcbits, xbar, stochastic)
        ctx.save_for_backward(x, w_q)
        return out

    _ARGS = _arg_names(forward.__func__)

    @staticmethod
    def backward(ctx, grad_output):
        gx, gw, ga, gsa = _cim_backward(ctx, grad_output, True)
        return _grads(_CimConv2dLSQ._ARGS, x=gx, w_q=gw, sa=gsa, alpha_q=ga)


def cim_conv2d_lsq(x, w_q, sa, sw, alpha_q, binary_mask, signed_act, stride, padding, dilation,
                   nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar, stochastic=False):
    """out[B, P, O] of the fused act-LSQ + CiM conv; differentiable in x, w_q, sa, alpha_q.
    ``stochastic``: the stochastic 1.5-bit ADC of lsq.py:205-221 in the forward.
    A call nothing can differentiate (inference_call) runs forward only and saves nothing."""
    if inference_call(x, w_q, sa, sw, alpha_q):
        return _CimConv2dLSQ._call(x, w_q, sa, sw, alpha_q, binary_mask, signed_act, stride, padding, dilation,
                                   nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar, stochastic, inference=True)[0]
    return _CimConv2dLSQ.apply(x, w_q, sa, sw, alpha_q, binary_mask, signed_act, stride, padding,
                               dilation, nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar, stochastic)


# ---------------------------------------------------------------------------------------------
# scale + shift ADC (test/test_backward_cimlayer_scale_shift.py)
# ---------------------------------------------------------------------------------------------
def _mask_int8(binary_mask, dev):
    bm = binary_mask.detach().to(device=dev)
    b8 = bm.to(torch.int8)
    if not torch.equal(b8.to(bm.dtype), bm):
        raise ValueError("binary_mask values must be int8 integers (as _Conv2dQCiM builds them)")
    return b8.contiguous()


def _shift_forward(ctx, x, w, sa, sw, alpha, beta, binary_mask, signed_act, stride, padding, dilation,
                   act_bits, act_bs, w_bits, w_bs, adc_bits, arr, variant, input_kind, qp_a):
    _require_device(x)
    dev = x.device
    B, C, H, W, O, KH, KW, st, pd, Ho, Wo = _geometry(x, w, stride, padding, dilation)
    desc = _lib.make_desc(B, C, H, W, O, KH, KW, st, pd, arr, w_bits, act_bits, w_bs, act_bs, adc_bits,
                          input_kind, qp_a, variant)
    sizes = _lib.query_sizes(desc)
    o = _operands(x, w, sa, sw, alpha, beta, _mask_int8(binary_mask, dev), signed_act)
    T = num_xbars(C, (KH, KW), arr)
    nbw, nba = int(w_bits / w_bs), int(act_bits / act_bs)
    if o.alpha.numel() != T * nbw * nba * O or o.beta.numel() != T * nbw * nba * O:
        o.alpha = o.alpha.expand(1, T, nbw, nba, 1, O).contiguous()
        o.beta = o.beta.expand(1, T, nbw, nba, 1, O).contiguous()
    out = torch.empty(B, Ho * Wo, O, device=dev, dtype=torch.float32)
    o.ctx = _ubuf(sizes.ctx_bytes, dev)
    _lib.check(_lib.load().cimq_shift_forward(desc, *_ptrs(o.x, o.w, o.sa, o.sw, o.alpha, o.beta, o.mask, o.sgn, out,
                                                           o.ctx), None, _stream()), "cimq_shift_forward")
    ctx.desc, ctx.sizes, ctx.bufs = desc, sizes, o
    return out


def _shift_backward(ctx, grad_output):
    ctx.saved_tensors  # noqa: B018 -- version check of x / w
    o = ctx.bufs
    dev = o.x.device
    g = _f32(grad_output, dev)
    gx = torch.empty_like(o.x)
    gw = torch.empty_like(o.w)
    ga = torch.empty_like(o.alpha)
    gb = torch.empty_like(o.beta)
    gsa = torch.empty(1, device=dev, dtype=torch.float32)
    ws = _ubuf(ctx.sizes.bwd_workspace_bytes, dev)
    _lib.check(_lib.load().cimq_shift_backward(ctx.desc, *_ptrs(g, o.x, o.sa, o.sw, o.alpha, o.beta, o.mask, o.sgn,
                                                                o.ctx, gx, gw, ga, gb, gsa, ws), _stream()),
               "cimq_shift_backward")
    # full [1, T, nbw, nba, 1, O]: autograd sums them down to a broadcast alpha / beta's own shape
    return gx, gw, ga, gb, gsa


class _ShiftTestFunction:
    """Shared body of the 14-argument scale + shift Functions of test_backward_cimlayer_scale_
    shift.py on integer inputs x_int / w_int (no LSQ scales): sa = sw = 1 on the device."""

    @staticmethod
    def _fwd(ctx, variant, x_int, w_int, conv_stride, conv_padding, conv_dilation, act_bits, act_bit_slice,
             weight_bits, weight_bit_slice, adc_bits, arr, binary_mask, alpha_cim, beta_cim):
        if int(weight_bits / weight_bit_slice) != int(act_bits / act_bit_slice):
            # the reference divides the act-slice grads with the weight-slice count as loop
            # bound (scale_shift.py:534): only nbw == nba is well defined there
            raise ValueError("the scale/shift Functions need as many weight as activation bit slices")
        one = torch.ones(1, device=x_int.device, dtype=torch.float32)
        zero = torch.zeros(1, device=x_int.device, dtype=torch.float32)
        ctx.save_for_backward(x_int, w_int)
        return _shift_forward(ctx, x_int, w_int, one, one, alpha_cim, beta_cim, binary_mask, zero, conv_stride,
                              conv_padding, conv_dilation, act_bits, act_bit_slice, weight_bits, weight_bit_slice,
                              adc_bits, arr, variant, _lib.CIMQ_INPUT_XQ, 0.0)

    @staticmethod
    def _bwd(ctx, grad_output, names):
        gx, gw, ga, gb, _ = _shift_backward(ctx, grad_output)
        return _grads(names, x_int=gx, w_int=gw, alpha_cim=ga, beta_cim=gb)


class get_analog_partial_sums_autograd_ver2(torch.autograd.Function):
    """Scale + shift ADC ``clamp(round((ps-beta)/alpha))*alpha + beta`` on int8-stored partial
    sums (test_backward_cimlayer_scale_shift.py:336-546): same 14 positional args, grads at 0, 1,
    12 (alpha_cim) and 13 (beta_cim)."""

    @staticmethod
    def forward(ctx, x_int, w_int, conv_stride, conv_padding, conv_dilation, act_bits, act_bit_slice,
                weight_bits, weight_bit_slice, adc_bits, arr, binary_mask, alpha_cim, beta_cim):
        v = _lib.CIMQ_ADC_SHIFT_ROUND | _lib.CIMQ_ADC_F_PS_INT8 | _lib.CIMQ_ADC_F_SHIFT_RANGE
        return _ShiftTestFunction._fwd(ctx, v, x_int, w_int, conv_stride, conv_padding, conv_dilation, act_bits,
                                       act_bit_slice, weight_bits, weight_bit_slice, adc_bits, arr, binary_mask,
                                       alpha_cim, beta_cim)

    _ARGS = _arg_names(forward.__func__)

    @staticmethod
    def backward(ctx, grad_output):
        return _ShiftTestFunction._bwd(ctx, grad_output, get_analog_partial_sums_autograd_ver2._ARGS)


class get_adcless_cim_output(torch.autograd.Function):
    """Scale + shift sign ADC ``sign((ps-beta)/alpha)*alpha + beta`` (test_backward_cimlayer_scale_
    shift.py:113-334): same 14 positional args, grads at 0, 1, 12 and 13."""

    @staticmethod
    def forward(ctx, x_int, w_int, conv_stride, conv_padding, conv_dilation, act_bits, act_bit_slice,
                weight_bits, weight_bit_slice, adc_bits, arr, binary_mask, alpha_cim, beta_cim):
        if adc_bits != 1:
            raise ValueError("get_adcless_cim_output is a 1-bit (sign) ADC")
        v = _lib.CIMQ_ADC_SHIFT_SIGN | _lib.CIMQ_ADC_F_SHIFT_RANGE
        return _ShiftTestFunction._fwd(ctx, v, x_int, w_int, conv_stride, conv_padding, conv_dilation, act_bits,
                                       act_bit_slice, weight_bits, weight_bit_slice, adc_bits, arr, binary_mask,
                                       alpha_cim, beta_cim)

    _ARGS = _arg_names(forward.__func__)

    @staticmethod
    def backward(ctx, grad_output):
        return _ShiftTestFunction._bwd(ctx, grad_output, get_adcless_cim_output._ARGS)


class _CimConv2dLSQShift(torch.autograd.Function):
    """Conv2dLSQCiM(adc_shift=True): fused act-LSQ + CiM conv whose ADC is the scale + shift one
    applied to the library's rescaled partial sum u = fp16(ps)*sw*sa (lsq.py:195)."""

    @staticmethod
    def forward(ctx, x, w_q, sa, sw, alpha_q, beta, binary_mask, signed_act, stride, padding, dilation,
                nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar):
        variant = _lib.CIMQ_ADC_SHIFT_SIGN if adcbits == 1 else _lib.CIMQ_ADC_SHIFT_ROUND
        ctx.save_for_backward(x, w_q)
        return _shift_forward(ctx, x, w_q, sa, sw, alpha_q, beta, binary_mask, signed_act, stride, padding,
                              dilation, nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar, variant,
                              _lib.CIMQ_INPUT_RAW_LSQ, float(2 ** nbits_a - 1))

    _ARGS = _arg_names(forward.__func__)

    @staticmethod
    def backward(ctx, grad_output):
        gx, gw, ga, gb, gsa = _shift_backward(ctx, grad_output)
        return _grads(_CimConv2dLSQShift._ARGS, x=gx, w_q=gw, sa=gsa, alpha_q=ga, beta=gb)


def cim_conv2d_lsq_shift(x, w_q, sa, sw, alpha_q, beta, binary_mask, signed_act, stride, padding, dilation,
                         nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar):
    """out[B, P, O] of the fused act-LSQ + scale/shift-ADC CiM conv; differentiable in x, w_q, sa,
    alpha_q and beta.  adcbits 1.5: clamp(round((u-beta)/alpha), -1, 1)*alpha + beta (ver2 on u);
    adcbits 1: sign((u-beta)/alpha)*alpha + beta (adcless on u)."""
    if adcbits not in (1, 1.5):
        raise ValueError("the scale/shift ADC option needs adcbits 1 or 1.5")
    return _CimConv2dLSQShift.apply(x, w_q, sa, sw, alpha_q, beta, binary_mask, signed_act, stride, padding,
                                    dilation, nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar)


class _ChainState:
    """The chained module backward of one device (cimq_module_backward_chain): the epilogues the
    calls left, the tensors each reads / writes (kept alive until it has been issued), the stream
    of the chain, and whether the end-of-backward flush is queued or a chained_epilogues() scope
    owns the flush."""

    def __init__(self):
        self.pending = _lib.Pending()
        self.keep = []
        self.stream = None
        self.queued = False
        self.scopes = 0

    def add(self, bufs):
        # a call that issued the earlier epilogues itself (a full list) leaves only its own
        if _lib.load().cimq_pending_jobs(self.pending) <= 1:
            self.keep = []
        self.keep.append(bufs)

    def flush(self):
        if self.keep:
            _lib.check(_lib.load().cimq_pending_flush(self.pending, self.stream), "cimq_pending_flush")
        self.keep = []
        self.queued = False


_CHAINS = {}
CHAIN_EPILOGUES = True  # tests switch it off to compare against the unchained backward


def _chain(dev):
    return _CHAINS.setdefault(dev.index if dev.index is not None else torch.cuda.current_device(), _ChainState())


@contextlib.contextmanager
def chained_epilogues(device=None):
    """Chain the parameter-gradient epilogues of Conv2dLSQCiM backwards across separate
    ``backward()`` calls made inside this scope (e.g. one per layer, as bench.py does): every
    layer's epilogue is held back and all are launched together, packed, when the scope ends.  Without a scope, a single backward pass chains its layers and flushes
    at its end (a queued autograd callback).  Applies to the in-place accumulating backward
    (GradBucket-owned layers); read the gradients only after the scope."""
    ch = _chain(torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device))
    ch.scopes += 1
    try:
        yield
    finally:
        ch.scopes -= 1
        if ch.scopes == 0:
            ch.flush()


class WeightPrep:
    """The weight side of one Conv2dLSQCiM forward, computed ahead by ``prepare_weights``
    (cimq_module_prepare): the buffer, the descriptors it was made for and the parameter
    versions it saw.  A forward takes it once (``_take_wprep``) if all three still match."""

    __slots__ = ("buf", "key", "versions")

    def __init__(self, buf, key, versions):
        self.buf, self.key, self.versions = buf, key, versions


def _prep_key(desc, lsq, x_shape):
    return (bytes(desc), lsq.qn_w, lsq.qp_w, lsq.gscale_a, lsq.gscale_w, lsq.nbits_alpha, tuple(x_shape))


def _versions(*ts):
    """Staleness key of a prepared weight side: each tensor's version counter and storage
    address.  An edit through ``p.data`` bumps neither; after one, call prepare_weights again
    (or torch.autograd.graph.increment_version(p)) before the next forward."""
    return tuple(-1 if t is None else (t._version, t.data_ptr()) for t in ts)


def _layer_params(m):
    """The tensors a prepared weight side of layer ``m`` depends on, in _versions' order (beta_cim for a
    shift-ADC layer alone)."""
    return (m.weight, m.alpha_act, m.alpha_weight, m.alpha_cim, m.binary_mask,
            m.beta_cim if getattr(m, "adc_shift", False) else None)


def _wprep_matches(wprep, desc, lsq, x_shape, params):
    """Whether ``wprep`` was made for exactly these descriptors, this input shape and the tensors ``params``
    (weight, alpha_act, alpha_weight, alpha_cim, binary_mask, beta_cim or None) as they are now."""
    return (wprep is not None and wprep.key == _prep_key(desc, lsq, x_shape)
            and wprep.versions == _versions(*params))


def _take_wprep(wprep, desc, lsq, x_shape, params, stochastic):
    """Hand a matching prepared weight side (prepare_weights / inference_weights) to the call ``lsq`` describes;
    returns the buffer the caller keeps alive across the call, or None.  A stochastic call never reads one."""
    if stochastic or not _wprep_matches(wprep, desc, lsq, x_shape, params):
        return None
    lsq.wprep = wprep.buf.data_ptr()
    return wprep.buf


def _module_descs(x_shape, weight, stride, padding, dilation, nbits_a, abitslice, nbits_w, wbitslice, adcbits,
                  xbar, nbits_alpha, has_alpha, stochastic, recompute=False, inference=False):
    B, C, H, W = x_shape
    O, _, KH, KW = weight.shape
    qp_a = float(2 ** nbits_a - 1)
    qn_w, qp_w = -(2 ** (nbits_w - 1)), 2 ** (nbits_w - 1) - 1
    desc = _lib.make_desc(B, C, H, W, O, KH, KW, _pair(stride), _pair(padding), xbar, nbits_w, nbits_a, wbitslice,
                          abitslice, adcbits, _lib.CIMQ_INPUT_RAW_LSQ, qp_a,
                          _lib.CIMQ_ADC_STOCHASTIC if stochastic else _lib.CIMQ_ADC_LIBRARY,
                          stochastic_seed() if stochastic else 0,
                          (_lib.CIMQ_OPT_RECOMPUTE if recompute else 0) | (_lib.CIMQ_OPT_INFERENCE if inference else 0))
    lsq = _lib.make_lsq_desc(qn_w, qp_w, 1.0 / math.sqrt(B * C * H * W * qp_a),
                             1.0 / math.sqrt(weight.numel() * qp_w), nbits_alpha if has_alpha else 0)
    return desc, lsq


def _shift_module_descs(x_shape, weight, stride, padding, dilation, nbits_a, abitslice, nbits_w, wbitslice, xbar,
                        nbits_alpha):
    desc, lsq = _module_descs(tuple(x_shape), weight, stride, padding, dilation, nbits_a, abitslice, nbits_w,
                              wbitslice, 1.5, xbar, nbits_alpha, True, False)
    desc.adc_variant = _lib.CIMQ_ADC_SHIFT_ROUND
    return desc, lsq


def _layer_descs(x_shape, weight, cfg, has_alpha, shift, stochastic=False, recompute=False, inference=False):
    """The descriptor pair of one module-entry-point call.  ``cfg``: (stride, padding, dilation, nbits_a, abitslice,
    nbits_w, wbitslice, adcbits, xbar, nbits_alpha), Conv2dLSQCiM.layer_config's order; ``shift``: the fused shift
    path's pair (adc 1.5, never stochastic, no recompute form)."""
    if shift:
        desc, lsq = _shift_module_descs(x_shape, weight, *cfg[:7], *cfg[8:])
        if inference:
            desc.options |= _lib.CIMQ_OPT_INFERENCE
        return desc, lsq
    return _module_descs(x_shape, weight, *cfg, has_alpha, stochastic, recompute, inference)


def module_descs(m, x_shape, inference=False):
    """The descriptor pair of layer ``m`` (a Conv2dLSQCiM) for input shape ``x_shape``: what its forward builds,
    what a prepared weight side is made for and what a route or size query asks about.  A shift-ADC layer
    (``m.adc_shift``): the fused shift path's pair.  Never the stochastic form, which would draw a seed."""
    return _layer_descs(x_shape, m.weight, m.layer_config(), m.alpha_cim is not None,
                        bool(getattr(m, "adc_shift", False)), False, bool(getattr(m, "recompute_psum", False)),
                        inference)


_prepare_descs = module_descs  # the name it had while it was private: kept for callers written against it


def _prepare_item(m, shape, inference=False):
    """One layer's cimq_module_prepare item for input shape ``shape``, what it must keep alive until the
    call, and the WeightPrep the call fills.  ``inference``: for the forward-only descriptor (the only one the
    library prepares a shift-ADC layer for)."""
    has_alpha = m.alpha_cim is not None
    shift = bool(getattr(m, "adc_shift", False))
    if shift and not inference:
        raise ValueError("a shift-ADC layer's weight side is prepared for forward-only calls alone")
    desc, lsq = module_descs(m, shape, inference)
    sizes = _lib.query_sizes(desc)
    dev = m.weight.device
    buf = _ubuf(sizes.wprep_bytes, dev)
    bm = m.binary_mask.to(device=dev, dtype=torch.int8).contiguous()
    params = _layer_params(m)
    for t in params[:4] + params[5:]:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError("prepare_weights: parameters must be contiguous fp32")
    it = _lib.PrepareShiftItem() if shift else _lib.PrepareItem()
    if shift:  # cimq_module_prepare_shift's item: beta_cim as well
        it.beta_cim = m.beta_cim.data_ptr()
    it.desc = ctypes.pointer(desc)
    it.lsq = ctypes.pointer(lsq)
    it.weight = m.weight.data_ptr()
    it.alpha_act = m.alpha_act.data_ptr()
    it.alpha_weight = m.alpha_weight.data_ptr()
    it.alpha_cim = m.alpha_cim.data_ptr() if has_alpha else None
    it.binary_mask = bm.data_ptr()
    it.wprep = buf.data_ptr()
    return it, (desc, lsq, bm), WeightPrep(buf, _prep_key(desc, lsq, shape), _versions(*params))


def inference_weights(m, x_shape, cached=None):
    """The weight side of a forward-only call of the fused Conv2dLSQCiM ``m`` on input shape ``x_shape``:
    ``cached`` if that WeightPrep was made for this shape and the parameters as they are now (_wprep_matches
    -- an edit through ``p.data`` bumps no version: drop the cache after one), else a new one from
    cimq_module_prepare with the forward roles only.  Conv2dLSQCiM keeps it across the batches of an evaluation.
    A shift-ADC layer (``m.adc_shift``, one the fused shift path takes): the same through
    cimq_module_prepare_shift, with beta_cim among the versions."""
    x_shape = tuple(x_shape)
    if cached is not None and _wprep_matches(cached, *module_descs(m, x_shape, inference=True), x_shape,
                                             _layer_params(m)):
        return cached
    it, keep, wp = _prepare_item(m, x_shape, inference=True)
    stream = torch.cuda.current_stream(m.weight.device).cuda_stream
    if getattr(m, "adc_shift", False):
        arr = (_lib.PrepareShiftItem * 1)(it)
        _lib.check(_lib.load().cimq_module_prepare_shift(1, arr, stream), "cimq_module_prepare_shift")
    else:
        arr = (_lib.PrepareItem * 1)(it)
        _lib.check(_lib.load().cimq_module_prepare(1, arr, stream), "cimq_module_prepare")
    del keep
    return wp


def prepare_weights(modules, stream=None):
    """Run the weight side of the next forward of every fused Conv2dLSQCiM in ``modules`` (the
    weight and alpha_cim quantisers into the CiM operands and ADC thresholds, lsq.py:552-571) in
    one library call, ahead of the forwards: each layer's forward then only quantises its
    activation.  Call it after the parameters are final for the step (after the optimizer step,
    before the forward pass); a forward whose parameters or input shape changed since, or that
    finds no prepared state, does the whole prologue itself, as without this call.  Layers still
    in their first (initialising) step, stochastic-ADC layers and non-fused paths are skipped."""
    items, keep, taken = [], [], []
    dev = None
    for m in modules:
        if not getattr(m, "_fused_ready", None) or not m._fused_ready():
            continue
        it, kp, wp = _prepare_item(m, m._last_x_shape)
        dev = m.weight.device
        items.append(it)
        keep.append(kp)
        taken.append((m, wp))
    if not items:
        return 0
    arr = (_lib.PrepareItem * len(items))(*items)
    s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    _lib.check(_lib.load().cimq_module_prepare(len(items), arr, s), "cimq_module_prepare")
    for m, wp in taken:
        m._wprep = wp
    return len(items)


class _LayerCall:
    """One call of a module entry point, ready to issue: the descriptor pair, the sizes, the operands (their ctx
    allocated), ``out`` (NCHW, ``out_shape``; None where the caller wants none), the forward workspace and the
    prepared weight side's buffer the call reads (``keep``, None without one)."""

    __slots__ = ("desc", "lsq", "sizes", "ops", "out", "out_shape", "ws", "keep")


def _layer_call(x, weight, alpha_act, alpha_weight, alpha_cim, beta_cim, binary_mask, signed_act, cfg,
                stochastic=False, wprep=None, recompute=False, inference=False, x_codes=False, want_out=True):
    """What cimq_module_forward, cimq_module_shift_forward (``beta_cim`` given), cimq_module_forward_epilogue and
    cimq_module_forward_codes have in common, for a layer of configuration ``cfg`` (_layer_descs).  ``wprep``: a
    WeightPrep, used only if it matches this call; a shift call that can be differentiated never reads one (the
    library's shift backward reads nothing prepared).  The ctx is the module entry points' (module_ctx_bytes:
    no per-partial-sum state words where the backward recomputes them, ABI 13)."""
    _require_device(x)
    dev = x.device
    B, _, _, _, O, _, _, st, pd, Ho, Wo = _geometry(x, weight, cfg[0], cfg[1], cfg[2])
    shift = beta_cim is not None
    c = _LayerCall()
    c.desc, c.lsq = _layer_descs(tuple(x.shape), weight, (st, pd) + cfg[2:], alpha_cim is not None, shift,
                                 stochastic, recompute, inference)
    c.keep = None
    if inference or not shift:
        c.keep = _take_wprep(wprep, c.desc, c.lsq, x.shape,
                             (weight, alpha_act, alpha_weight, alpha_cim, binary_mask, beta_cim), stochastic)
    c.sizes = _lib.query_sizes(c.desc)
    c.ops = _operands(x, weight, alpha_act, alpha_weight, alpha_cim, beta_cim, binary_mask, signed_act, x_codes)
    c.out_shape = (B, O, Ho, Wo)
    c.out = torch.empty(c.out_shape, device=dev, dtype=torch.float32) if want_out else None
    c.ops.ctx = _ubuf(c.sizes.module_ctx_bytes, dev)
    c.ws = _ubuf(c.sizes.fwd_workspace_bytes, dev)
    return c


def _param_grad_bufs(o):
    """Fresh gradient buffers for weight, alpha_act, alpha_weight, alpha_cim and beta_cim (None where the layer
    has none) of a module backward on the operands ``o``."""
    dev = o.x.device
    return (torch.empty_like(o.w), torch.empty(1, device=dev, dtype=torch.float32),
            torch.empty(1, device=dev, dtype=torch.float32),
            None if o.alpha is None else torch.empty_like(o.alpha),
            None if o.beta is None else torch.empty_like(o.beta))


class _CimModuleConv(torch.autograd.Function):
    """A whole Conv2dLSQCiM layer after its first-step init (lsq.py:544-581): the activation,
    weight and alpha_cim quantisers run inside libcimq on the raw parameters (no torch ops,
    no materialised x_q / w_q / alpha_q tensors); returns the NCHW output.

    With ``accumulate`` set, the backward adds the parameter gradients straight into the
    parameters' existing ``.grad`` buffers inside the library (what torch's AccumulateGrad
    would do, without its four extra add kernels) and returns None for them.  It does so only
    when all four ``.grad`` buffers exist as contiguous fp32 device tensors; otherwise the
    gradients are returned as usual.  Parameter hooks (e.g. DistributedDataParallel's) do not
    fire for in-place accumulated gradients, so this is for callers that own the gradient
    exchange, like ``dist.GradBucket``.  ``tail_stream`` (accumulate mode only): the parameter-
    gradient epilogue runs there, off the grad_x chain, ordered after this backward by an event;
    the bucket joins that stream before it reads the gradients (GradBucket.join)."""

    @staticmethod
    def _call(x, weight, alpha_act, alpha_weight, alpha_cim, binary_mask, signed_act, stride, padding, dilation,
              nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar, nbits_alpha, stochastic=False, wprep=None,
              recompute=False, inference=False):
        """cimq_module_forward; returns its _LayerCall.  ``inference``: CIMQ_OPT_INFERENCE (the small ctx and the
        forward workspace, dropped by the caller)."""
        c = _layer_call(x, weight, alpha_act, alpha_weight, alpha_cim, None, binary_mask, signed_act,
                        (stride, padding, dilation, nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar, nbits_alpha),
                        stochastic, wprep, recompute, inference)
        o = c.ops
        _lib.check(_lib.load().cimq_module_forward(c.desc, c.lsq, *_ptrs(o.x, o.w, o.sa, o.sw, o.alpha, o.mask, o.sgn,
                                                                         c.out, o.ctx, c.ws), _stream()),
                   "cimq_module_forward")
        return c

    @staticmethod
    def forward(ctx, x, weight, alpha_act, alpha_weight, alpha_cim, binary_mask, signed_act, stride, padding,
                dilation, nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar, nbits_alpha, accumulate=False,
                stochastic=False, tail_stream=None, wprep=None, recompute=False):
        c = _CimModuleConv._call(
            x, weight, alpha_act, alpha_weight, alpha_cim, binary_mask, signed_act, stride, padding, dilation, nbits_a,
            abitslice, nbits_w, wbitslice, adcbits, xbar, nbits_alpha, stochastic, wprep, recompute)
        ctx.desc, ctx.lsq, ctx.sizes, ctx.bufs, ctx.wprep_buf = c.desc, c.lsq, c.sizes, c.ops, c.keep
        ctx.module_path = True  # a cimq_module_forward ctx (debug_state_codes)
        # the backward reads x and the raw parameters again (act-LSQ / weight-LSQ STE); saving
        # them lets autograd's version counters catch an in-place change in between
        ctx.save_for_backward(x, weight, alpha_act, alpha_weight, alpha_cim)
        ctx.params = (weight, alpha_act, alpha_weight, alpha_cim) if accumulate else None
        ctx.tail_stream = tail_stream if accumulate else None
        return c.out

    _ARGS = _arg_names(forward.__func__)

    @staticmethod
    def _grad_targets(ctx):
        """The parameters' .grad buffers when the backward may accumulate into them."""
        if ctx.params is None:
            return None
        grads = []
        for p in ctx.params:
            if p is None:
                grads.append(None)
                continue
            g = p.grad
            if (g is None or g.dtype != torch.float32 or not g.is_contiguous() or g.device != p.device
                    or g.shape != p.shape):
                return None
            grads.append(g)
        return grads

    @staticmethod
    def backward(ctx, grad_output):
        ctx.saved_tensors  # noqa: B018 -- version check of x and the parameters
        o = ctx.bufs
        dev = o.x.device
        g = _f32(grad_output, dev)
        gx = torch.empty_like(o.x)
        targets = _CimModuleConv._grad_targets(ctx)
        lsq = ctx.lsq
        side = ctx.tail_stream if targets is not None else None
        if targets is not None:
            gw, gaa, gaw, gac = targets
            lsq = _lib.make_lsq_desc(lsq.qn_w, lsq.qp_w, lsq.gscale_a, lsq.gscale_w, lsq.nbits_alpha,
                                     _lib.CIMQ_LSQ_ACCUMULATE_GRADS | (_lib.CIMQ_LSQ_DEFER_GW if side else 0),
                                     lsq.wprep)
        else:
            gw, gaa, gaw, gac, _ = _param_grad_bufs(o)
        ws = _ubuf(ctx.sizes.bwd_workspace_bytes, dev)
        lib = _lib.load()
        # cimq_module_backward's arguments up to the workspace; cimq_module_backward_chain takes the same
        args = [ctx.desc, lsq] + _ptrs(g, o.x, o.w, o.sa, o.sw, o.alpha, o.mask, o.sgn, o.ctx, gx, gw, gaa, gaw, gac,
                                       ws)
        if targets is not None and side is None and CHAIN_EPILOGUES:
            # chained: this layer's epilogue waits in the pending list; the flush launches all of
            # them packed into a few launches
            ch = _chain(dev)
            stream = _stream()
            if ch.keep and ch.stream != stream:
                ch.flush()
            if ch.scopes == 0 and not ch.queued:
                torch.autograd.Variable._execution_engine.queue_callback(ch.flush)
                ch.queued = True
            ch.stream = stream
            _lib.check(lib.cimq_module_backward_chain(*args, ch.pending, stream), "cimq_module_backward_chain")
            ch.add((ws, o.ctx, o.w, o.alpha, gw, gaa, gaw, gac, ctx.wprep_buf))
            return _grads(_CimModuleConv._ARGS, x=gx)
        _lib.check(lib.cimq_module_backward(*args, _stream()), "cimq_module_backward")
        if side is not None:
            # the parameter-gradient half (the grad_w kernel of the v7 layers, then the epilogue) on
            # the bucket's stream: the next layer's backward does not wait for it; grad_out / ws /
            # ctx stay alive until that stream is done with them
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                _lib.check(lib.cimq_module_backward_params(ctx.desc, lsq, *_ptrs(g, o.w, o.alpha, o.ctx, gw, gaa, gaw,
                                                                                 gac, ws), side.cuda_stream),
                           "cimq_module_backward_params")
            for t in (g, ws, o.ctx, o.w, o.alpha, ctx.wprep_buf):
                if t is not None:
                    t.record_stream(side)
        if targets is not None:
            return _grads(_CimModuleConv._ARGS, x=gx)
        return _grads(_CimModuleConv._ARGS, x=gx, weight=gw, alpha_act=gaa, alpha_weight=gaw, alpha_cim=gac)


def cim_module_conv(x, weight, alpha_act, alpha_weight, alpha_cim, binary_mask, signed_act, stride, padding,
                    dilation, nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar, nbits_alpha,
                    accumulate=False, stochastic=False, tail_stream=None, wprep=None, recompute=False):
    """NCHW output of a Conv2dLSQCiM layer (quantisers fused); differentiable in x, weight and
    the three step-size parameters (alpha_act and alpha_weight are 1-element tensors).
    ``accumulate`` / ``tail_stream``: see _CimModuleConv; ``stochastic``: the stochastic 1.5-bit ADC;
    ``wprep``: a WeightPrep from prepare_weights (used only if it matches this call); ``recompute``:
    CIMQ_OPT_RECOMPUTE (no state words in the ctx where a recompute backward exists; slower).
    A call nothing can differentiate (inference_call) runs forward only (CIMQ_OPT_INFERENCE): out, the small
    ctx and the forward workspace are allocated, nothing is saved; ``wprep`` then comes from inference_weights."""
    if inference_call(x, weight, alpha_act, alpha_weight, alpha_cim):
        return _CimModuleConv._call(x, weight, alpha_act, alpha_weight, alpha_cim, binary_mask, signed_act, stride,
                                    padding, dilation, nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar,
                                    nbits_alpha, stochastic, wprep, recompute, inference=True).out
    return _CimModuleConv.apply(x, weight, alpha_act, alpha_weight, alpha_cim, binary_mask, signed_act, stride,
                                padding, dilation, nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar,
                                nbits_alpha, accumulate, stochastic, tail_stream, wprep, recompute)


def module_shift_supported(x_shape, weight, stride, padding, dilation, nbits_a, abitslice, nbits_w, wbitslice,
                           adcbits, xbar, nbits_alpha):
    """Whether cim_module_shift_conv takes this Conv2dLSQCiM(adc_shift=True) layer (libcimq's fused
    shift path: adc 1.5, 2 or 3 equal slices, a fast-path conv shape); else the module quantises in
    torch and calls the unfused shift entry points."""
    if adcbits != 1.5 or len(x_shape) != 4:
        return False
    if _pair(dilation) != (1, 1):
        return False
    desc, _ = _shift_module_descs(x_shape, weight, stride, padding, dilation, nbits_a, abitslice, nbits_w, wbitslice,
                                  xbar, nbits_alpha)
    return bool(_lib.load().cimq_module_shift_supported(desc))


class _CimModuleShiftConv(torch.autograd.Function):
    """Conv2dLSQCiM(adc_shift=True) after its first-step init: as _CimModuleConv (activation, weight and
    alpha_cim quantisers inside libcimq), with the scale + shift ADC of test_backward_cimlayer_scale_
    shift.py:336-546 on the rescaled partial sum; differentiable in x, weight, alpha_act, alpha_weight,
    alpha_cim and beta_cim.  NCHW output."""

    @staticmethod
    def _call(x, weight, alpha_act, alpha_weight, alpha_cim, beta_cim, binary_mask, signed_act, stride,
              padding, dilation, nbits_a, abitslice, nbits_w, wbitslice, xbar, nbits_alpha, inference=False,
              wprep=None):
        """cimq_module_shift_forward; returns its _LayerCall.  ``wprep`` (a forward-only call alone): a WeightPrep
        from inference_weights, used if it was made for exactly this call."""
        c = _layer_call(x, weight, alpha_act, alpha_weight, alpha_cim, beta_cim, binary_mask, signed_act,
                        (stride, padding, dilation, nbits_a, abitslice, nbits_w, wbitslice, 1.5, xbar, nbits_alpha),
                        wprep=wprep, inference=inference)
        o = c.ops
        _lib.check(_lib.load().cimq_module_shift_forward(
            c.desc, c.lsq, *_ptrs(o.x, o.w, o.sa, o.sw, o.alpha, o.beta, o.mask, o.sgn, c.out, o.ctx, c.ws), _stream()),
            "cimq_module_shift_forward")
        return c

    @staticmethod
    def forward(ctx, x, weight, alpha_act, alpha_weight, alpha_cim, beta_cim, binary_mask, signed_act, stride,
                padding, dilation, nbits_a, abitslice, nbits_w, wbitslice, xbar, nbits_alpha):
        c = _CimModuleShiftConv._call(
            x, weight, alpha_act, alpha_weight, alpha_cim, beta_cim, binary_mask, signed_act, stride, padding,
            dilation, nbits_a, abitslice, nbits_w, wbitslice, xbar, nbits_alpha)
        ctx.desc, ctx.lsq, ctx.sizes, ctx.bufs = c.desc, c.lsq, c.sizes, c.ops
        ctx.save_for_backward(x, weight, alpha_act, alpha_weight, alpha_cim, beta_cim)
        return c.out

    _ARGS = _arg_names(forward.__func__)

    @staticmethod
    def backward(ctx, grad_output):
        ctx.saved_tensors  # noqa: B018 -- version check of x and the parameters
        o = ctx.bufs
        dev = o.x.device
        g = _f32(grad_output, dev)
        gx = torch.empty_like(o.x)
        gw, gaa, gaw, gac, gbc = _param_grad_bufs(o)
        ws = _ubuf(ctx.sizes.bwd_workspace_bytes, dev)
        _lib.check(_lib.load().cimq_module_shift_backward(
            ctx.desc, ctx.lsq, *_ptrs(g, o.x, o.w, o.sa, o.sw, o.alpha, o.beta, o.mask, o.sgn, o.ctx, gx, gw, gaa, gaw,
                                      gac, gbc, ws), _stream()), "cimq_module_shift_backward")
        return _grads(_CimModuleShiftConv._ARGS, x=gx, weight=gw, alpha_act=gaa, alpha_weight=gaw, alpha_cim=gac,
                      beta_cim=gbc)


def cim_module_shift_conv(x, weight, alpha_act, alpha_weight, alpha_cim, beta_cim, binary_mask, signed_act, stride,
                          padding, dilation, nbits_a, abitslice, nbits_w, wbitslice, xbar, nbits_alpha, wprep=None):
    """NCHW output of a Conv2dLSQCiM(adc_shift=True, adcbits=1.5) layer with its quantisers fused
    (module_shift_supported must hold).  Forward only for a call nothing can differentiate (inference_call);
    ``wprep`` then comes from inference_weights (a call that can be differentiated never reads it)."""
    if inference_call(x, weight, alpha_act, alpha_weight, alpha_cim, beta_cim):
        return _CimModuleShiftConv._call(x, weight, alpha_act, alpha_weight, alpha_cim, beta_cim, binary_mask,
                                         signed_act, stride, padding, dilation, nbits_a, abitslice, nbits_w,
                                         wbitslice, xbar, nbits_alpha, inference=True, wprep=wprep).out
    return _CimModuleShiftConv.apply(x, weight, alpha_act, alpha_weight, alpha_cim, beta_cim, binary_mask,
                                     signed_act, stride, padding, dilation, nbits_a, abitslice, nbits_w, wbitslice,
                                     xbar, nbits_alpha)


def cim_module_conv_epilogue(x, weight, alpha_act, alpha_weight, alpha_cim, binary_mask, signed_act, stride, padding,
                             dilation, nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar, nbits_alpha, scale, shift,
                             residual=None, relu=False, beta_cim=None, stochastic=False, wprep=None, recompute=False):
    """cim_module_conv (``beta_cim`` None) or cim_module_shift_conv (``beta_cim`` given) of a call nothing can
    differentiate, with a per-channel epilogue applied in the registers of the kernel that stores the output
    (cimq_module_forward_epilogue, ABI 16): ``out = relu?(conv * scale[o] + shift[o] + residual?)``, each step one
    IEEE fp32 operation in that order -- bit for bit what ``torch.relu(conv * scale.view(1, -1, 1, 1) +
    shift.view(1, -1, 1, 1) + residual)`` gives on cim_module_conv's output.  ``scale`` / ``shift``: [O] fp32 device
    tensors (a folded BatchNorm); ``residual``: NCHW like the output, made contiguous fp32 if it is not.  Forward
    only: a call that could be differentiated raises RuntimeError."""
    return _conv_epilogue(x, weight, alpha_act, alpha_weight, alpha_cim, binary_mask, signed_act, stride, padding,
                          dilation, nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar, nbits_alpha, scale, shift,
                          residual, relu, beta_cim, stochastic, wprep, recompute, "cim_module_conv_epilogue")


def cim_module_conv_pool(x, weight, alpha_act, alpha_weight, alpha_cim, binary_mask, signed_act, stride, padding,
                         dilation, nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar, nbits_alpha, scale, shift,
                         residual=None, relu=False, pool=_lib.CIMQ_POOL_MAX2, wprep=None, recompute=False):
    """cim_module_conv_epilogue whose kernel stores the 2x2 / stride-2 max pool of the epilogue's values
    (cimq_module_forward_pool, ``pool`` CIMQ_POOL_MAX2): [B, O, Ho/2, Wo/2], bit for bit
    ``F.max_pool2d(cim_module_conv_epilogue(...), 2, 2)``.  ``residual`` keeps the unpooled shape.  ``pool`` 0 is
    cim_module_conv_epilogue.  Layers off the wide route, or wider than 32 output columns, raise CimqError
    (``_lib.module_pool_supported``)."""
    return _conv_epilogue(x, weight, alpha_act, alpha_weight, alpha_cim, binary_mask, signed_act, stride, padding,
                          dilation, nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar, nbits_alpha, scale, shift,
                          residual, relu, None, False, wprep, recompute, "cim_module_conv_pool", pool=int(pool))


def act_code_step(alpha_act, gscale_a):
    """The step size ``sa`` of a layer's activation quantiser as libcimq computes it: grad_scale's forward value
    ``(alpha_act - alpha_act * s) + alpha_act * s`` with every operation in fp32 (cimq_device.h grad_scale_value)."""
    a = alpha_act.detach().reshape(-1)[:1].to(torch.float32)
    yg = a * torch.tensor(gscale_a, dtype=torch.float32, device=a.device)
    return (a - yg) + yg


def act_codes_of(y, alpha_act, gscale_a, qp):
    """The torch twin of libcimq's activation code (include/cimq.h, cimq_act_codes) for an fp32 tensor ``y``
    entering a layer with step-size parameter ``alpha_act``, gradient-scale factor ``gscale_a`` and clamp maximum
    ``qp``: ``rint(clamp(y / sa, 0, qp))`` as uint8, ``qp + 1`` where y is NaN.  Runs on y's device; a CPU's fp32
    division is IEEE."""
    sa = act_code_step(alpha_act, gscale_a).to(y.device)
    r = torch.round(torch.clamp(y.to(torch.float32) / sa, 0.0, float(qp)))
    return torch.where(torch.isnan(r), torch.full_like(r, float(qp) + 1.0), r).to(torch.uint8)


def cim_module_conv_codes(x, weight, alpha_act, alpha_weight, alpha_cim, binary_mask, signed_act, stride, padding,
                          dilation, nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar, nbits_alpha, scale, shift,
                          residual=None, relu=False, beta_cim=None, stochastic=False, wprep=None, recompute=False,
                          out_quant=None, keep_float=True):
    """cim_module_conv_epilogue with activations as codes on either side (cimq_module_forward_codes).  ``x``: the
    fp32 input, or a ``torch.uint8`` tensor [B, C, H, W] of this layer's activation codes (act_codes_of with its
    alpha_act, its gradient-scale factor and Qp = 2^nbits_a - 1) -- the output is then bit for bit that of any fp32
    input with these codes.  ``out_quant``: None, or ``(alpha_act, gscale_a, qp)`` of the layer that consumes the
    output; the codes of the stored values for that layer are written by the kernel that stores them.  Returns the
    fp32 output (``out_quant`` None), ``(output, codes)``, or with ``keep_float=False`` the codes alone (the fp32
    output is then never written).  Forward only: a call that could be differentiated raises RuntimeError."""
    return _conv_epilogue(x, weight, alpha_act, alpha_weight, alpha_cim, binary_mask, signed_act, stride, padding,
                          dilation, nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar, nbits_alpha, scale, shift,
                          residual, relu, beta_cim, stochastic, wprep, recompute, "cim_module_conv_codes",
                          True, out_quant, keep_float)


def _conv_epilogue(x, weight, alpha_act, alpha_weight, alpha_cim, binary_mask, signed_act, stride, padding, dilation,
                   nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar, nbits_alpha, scale, shift, residual, relu,
                   beta_cim, stochastic, wprep, recompute, who, codes=False, out_quant=None, keep_float=True, pool=None):
    """The shared body of cim_module_conv_epilogue (``codes`` False: cimq_module_forward_epilogue, fp32 in and
    out), cim_module_conv_pool (``pool`` an int: cimq_module_forward_pool) and cim_module_conv_codes
    (cimq_module_forward_codes)."""
    if not inference_call(x, weight, alpha_act, alpha_weight, alpha_cim, beta_cim, scale, shift, residual):
        raise RuntimeError(f"{who} is forward only: call it under torch.no_grad(), or with no "
                           "argument that requires a gradient")
    _require_device(x)
    x_codes = codes and x.dtype == torch.uint8
    if not codes and (x.dtype == torch.uint8 or out_quant is not None):
        raise ValueError(f"{who}: fp32 in and out (activation codes: cim_module_conv_codes)")
    if out_quant is None and not keep_float:
        raise ValueError(f"{who}: keep_float=False needs out_quant")
    dev = x.device
    c = _layer_call(x, weight, alpha_act, alpha_weight, alpha_cim, beta_cim, binary_mask, signed_act,
                    (stride, padding, dilation, nbits_a, abitslice, nbits_w, wbitslice, adcbits, xbar, nbits_alpha),
                    stochastic, wprep, recompute, True, x_codes, keep_float)
    o, O = c.ops, c.out_shape[1]
    sc, sh = _f32(scale, dev).reshape(-1), _f32(shift, dev).reshape(-1)
    if sc.numel() != O or sh.numel() != O:
        raise ValueError(f"{who}: scale / shift need {O} elements (one per output channel)")
    rs = None
    if residual is not None:
        if tuple(residual.shape) != c.out_shape:
            raise ValueError(f"{who}: residual {tuple(residual.shape)} is not the output's "
                             f"{c.out_shape}")
        rs = _f32(residual, dev)
    epi = _lib.make_epilogue(*_ptrs(sc, sh, rs), relu)
    if pool:  # (any non-zero value reaches the library, which refuses all but CIMQ_POOL_MAX2)
        B, _, Ho, Wo = c.out_shape
        c.out = torch.empty((B, O, Ho // 2, Wo // 2), device=dev, dtype=torch.float32)
    # the operands every one of the two entry points takes between its leading arguments and the epilogue
    args = _ptrs(o.w, o.sa, o.sw, o.alpha, o.beta, o.mask, o.sgn) + [ctypes.byref(epi)] + _ptrs(c.out, o.ctx, c.ws) + \
        [_stream()]
    if pool is not None:
        _lib.check(_lib.load().cimq_module_forward_pool(c.desc, c.lsq, o.x.data_ptr(), *args[:8], pool, *args[8:]),
                   "cimq_module_forward_pool")
        return c.out
    if not codes:
        _lib.check(_lib.load().cimq_module_forward_epilogue(c.desc, c.lsq, o.x.data_ptr(), *args),
                   "cimq_module_forward_epilogue")
        return c.out
    oq = oa = None
    if out_quant is None:
        io = _lib.make_act_codes(x_codes=o.x.data_ptr() if x_codes else None)
    else:
        o_alpha, o_gs, o_qp = out_quant
        oa = o_alpha  # (a layer's own fp32 parameter on this device is read where it is)
        if not (oa.dtype == torch.float32 and oa.device == dev and oa.is_contiguous()):
            oa = _one(o_alpha, dev)
        oq = torch.empty(c.out_shape, device=dev, dtype=torch.uint8)
        io = _lib.make_act_codes(o.x.data_ptr() if x_codes else None, oq.data_ptr(), oa.data_ptr(), float(o_gs),
                                 float(o_qp), not keep_float)
    _lib.check(_lib.load().cimq_module_forward_codes(c.desc, c.lsq, ctypes.byref(io),
                                                     None if x_codes else o.x.data_ptr(), *args),
               "cimq_module_forward_codes")
    if oq is None:
        return c.out
    return (c.out, oq) if keep_float else oq


def net_sizes(net, ext=None):
    """cimq_net_sizes of a ``_lib.NetDesc``: (float bytes per slot, code bytes per slot, workspace bytes).  Raises
    CimqError where the library refuses the plan.  ``ext``: a ``_lib.NetExt`` (pooled layers, the flatten head):
    cimq_net_sizes_ex."""
    n = max(int(net.n_slots), 1)
    fb, cb, ws = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)(), ctypes.c_size_t()
    if ext is None:
        _lib.check(_lib.load().cimq_net_sizes(ctypes.byref(net), fb, cb, ctypes.byref(ws)), "cimq_net_sizes")
    else:
        _lib.check(_lib.load().cimq_net_sizes_ex(ctypes.byref(net), fb, cb, ctypes.byref(ws), ctypes.byref(ext)),
                   "cimq_net_sizes_ex")
    return list(fb)[:net.n_slots], list(cb)[:net.n_slots], ws.value


def net_forward(net, x, slot_float, slot_codes, logits, ws, stream=None, ext=None):
    """cimq_net_forward: the whole plan ``net`` (a ``_lib.NetDesc``) on ``stream`` (default: torch's current one) in
    one library call.  ``x`` / ``logits`` / ``ws``: device addresses (None where the plan has no use for one);
    ``slot_float`` / ``slot_codes``: ``(ctypes.c_void_p * n_slots)`` arrays of device addresses.  ``ext``: a
    ``_lib.NetExt``: cimq_net_forward_ex."""
    s = _stream() if stream is None else stream
    if ext is None:
        _lib.check(_lib.load().cimq_net_forward(ctypes.byref(net), x, slot_float, slot_codes, logits, ws, s),
                   "cimq_net_forward")
    else:
        _lib.check(_lib.load().cimq_net_forward_ex(ctypes.byref(net), x, slot_float, slot_codes, logits, ws, s,
                                                   ctypes.byref(ext)), "cimq_net_forward_ex")


def alpha_cim_init(x, w_q, sa, sw, binary_mask, signed_act, stride, padding, nbits_a, abitslice,
                   nbits_w, wbitslice, adcbits, xbar, num_xbars):
    """First-step alpha_cim initialisation on the device (lsq.py:557-563, 35-87)."""
    _require_device(x)
    dev = x.device
    B, C, H, W, O, KH, KW, st, pd, _, _ = _geometry(x, w_q, stride, padding, (1, 1))
    desc = _lib.make_desc(B, C, H, W, O, KH, KW, st, pd, xbar, nbits_w, nbits_a, wbitslice, abitslice,
                          adcbits, _lib.CIMQ_INPUT_RAW_LSQ, float(2 ** nbits_a - 1))
    sizes = _lib.query_sizes(desc)
    nbw, nba = int(nbits_w / wbitslice), int(nbits_a / abitslice)
    out = torch.empty(1, num_xbars, nbw, nba, 1, O, device=dev, dtype=torch.float32)
    o = _operands(x, w_q, sa, sw, None, None, binary_mask, signed_act)
    o.ctx = _ubuf(sizes.ctx_bytes, dev)
    ws = _ubuf(sizes.fwd_workspace_bytes, dev)
    _lib.check(_lib.load().cimq_alpha_init(desc, *_ptrs(o.x, o.w, o.sa, o.sw, o.mask, o.sgn, out, o.ctx, ws),
                                           _stream()), "cimq_alpha_init")
    return out


def debug_partial_sums(x_q, w_q, conv_stride, conv_padding, act_bits, act_bit_slice, weight_bits,
                       weight_bit_slice, adc_bits, arr, binary_mask, alpha_cim, weight_scaling_factor,
                       act_scaling_factor, signed_act, stochastic=False, seed=None):
    """Forward on the device that also returns the integer partial sums [B,T,nbw,nba,P,O]
    (int32) and the ADC outputs (fp32) -- the reference's ctx.ps_int / adc_out
    (lsq.py:169-230).  Parity-test hook; ``stochastic`` (with an optional Philox ``seed``)
    draws the stochastic ADC of lsq.py:205-221."""
    _require_device(x_q)
    dev = x_q.device
    B, C, H, W, O, KH, KW, st, pd, Ho, Wo = _geometry(x_q, w_q, conv_stride, conv_padding, (1, 1))
    desc = _lib.make_desc(B, C, H, W, O, KH, KW, st, pd, arr, weight_bits, act_bits, weight_bit_slice,
                          act_bit_slice, adc_bits, _lib.CIMQ_INPUT_XQ,
                          adc_variant=_lib.CIMQ_ADC_STOCHASTIC if stochastic else _lib.CIMQ_ADC_LIBRARY,
                          seed=(stochastic_seed() if seed is None else seed) if stochastic else 0)
    sizes = _lib.query_sizes(desc)
    nbw, nba = int(weight_bits / weight_bit_slice), int(act_bits / act_bit_slice)
    T = num_xbars(C, (KH, KW), arr)
    out = torch.empty(B, Ho * Wo, O, device=dev, dtype=torch.float32)
    ps = torch.zeros(B, T, nbw, nba, Ho * Wo, O, device=dev, dtype=torch.int32)
    adc = torch.zeros(B, T, nbw, nba, Ho * Wo, O, device=dev, dtype=torch.float32)
    o = _operands(x_q, w_q, act_scaling_factor, weight_scaling_factor, alpha_cim, None, binary_mask, signed_act)
    o.ctx = _ubuf(sizes.ctx_bytes, dev)
    _lib.check(_lib.load().cimq_debug_partial_sums(desc, *_ptrs(o.x, o.w, o.sa, o.sw, o.alpha, o.mask, o.sgn, out, ps,
                                                                adc, o.ctx), _stream()), "cimq_debug_partial_sums")
    return out, ps, adc


def debug_state_codes(out):
    """ADC codes (int8) and STE-pass bits (uint8) [B, T, nbw, nba, P, O] of every partial sum that
    the production forward (cim_fwd_v3_kernel, v7 path) recorded for ``out`` -- the output of
    get_cim_output_signed / cim_conv2d_lsq / cim_module_conv whose backward has not run yet.
    Parity-test hook (cimq_debug_state_codes)."""
    ctx = out.grad_fn
    while ctx is not None and not hasattr(ctx, "desc"):  # through views (the module's NCHW reshape)
        ctx = ctx.next_functions[0][0] if ctx.next_functions else None
    if ctx is None:
        raise RuntimeError("no libcimq forward context behind this tensor")
    d, o = ctx.desc, ctx.bufs
    dev = o.ctx.device
    nbw, nba = int(d.bits_w / d.bs_w), int(d.bits_a / d.bs_a)
    T = num_xbars(d.in_channels, (d.kernel_h, d.kernel_w), d.xbar)
    Ho, Wo = out_hw(d)
    shape = (d.batch, T, nbw, nba, Ho * Wo, d.out_channels)
    code = torch.empty(shape, device=dev, dtype=torch.int8)
    passed = torch.empty(shape, device=dev, dtype=torch.uint8)
    if getattr(ctx, "module_path", False) and _lib.module_route(d)[1] == _lib.CIMQ_ROUTE_R6:
        # a module layer whose backward recomputes the partial sums: its forward left no state words, so the
        # codes come from the recomputing backward's own code path (cimq_debug_recompute_codes)
        st = torch.empty(T * d.batch * Ho * Wo * d.out_channels * 4, device=dev, dtype=torch.uint8)
        _lib.check(_lib.load().cimq_debug_recompute_codes(d, *_ptrs(o.x, o.sgn, o.ctx, st, code, passed), _stream()),
                   "cimq_debug_recompute_codes")
        return code, passed
    _lib.check(_lib.load().cimq_debug_state_codes(d, *_ptrs(o.ctx, code, passed), _stream()), "cimq_debug_state_codes")
    return code, passed


def logical_macs(B, C, H, W, O, KH, KW, stride, padding) -> int:
    """ptflops convention B*Ho*Wo*O*C*KH*KW (utils/ptflops/flops_counter.py:314-318)."""
    Ho, Wo = conv_out_hw(H, W, KH, KW, stride, padding)
    return B * Ho * Wo * O * C * KH * KW


def num_xbars(in_channels, kernel_size, xbar) -> int:
    return int(math.ceil(in_channels * kernel_size[0] * kernel_size[1] / xbar))


# =============================================================================================
# plain LSQ modules (lsq.py:389-436 Conv2dLSQ, :591-617 LinearLSQ, :620-662 ActLSQ)
# =============================================================================================
_LSQ_WS = {}  # cimq_lsq_quantize_workspace_bytes per element count


class _LsqQuantize(torch.autograd.Function):
    """out = round_pass(clamp(x / s, qn, qp)) [* s] with s the grad-scaled step size (a [1]
    tensor: grad_scale(alpha, g) evaluated by torch, so its graph back to alpha stays torch's).
    Backward: grad_x and d loss / d s from libcimq (cimq_lsq_quantize_backward)."""

    @staticmethod
    def forward(ctx, x, s, qn, qp, scaled):
        _require_device(x, s)
        xc = x.detach().float().contiguous()
        sc = s.detach().float().reshape(-1)[:1].contiguous()
        out = torch.empty_like(xc)
        _lib.check(_lib.load().cimq_lsq_quantize_forward(xc.data_ptr(), xc.numel(), sc.data_ptr(), float(qn),
                                                         float(qp), 1 if scaled else 0, out.data_ptr(), _stream()),
                   "cimq_lsq_quantize_forward")
        ctx.save_for_backward(xc, sc)
        ctx.q = (float(qn), float(qp), 1 if scaled else 0)
        ctx.s_shape = s.shape
        return out

    @staticmethod
    def backward(ctx, g):
        xc, sc = ctx.saved_tensors
        qn, qp, scaled = ctx.q
        lib = _lib.load()
        gc = g.float().contiguous()
        gx = torch.empty_like(xc)
        gs = torch.empty(1, device=xc.device, dtype=torch.float32)
        n = xc.numel()
        nb = _LSQ_WS.get(n)
        if nb is None:
            nb = _LSQ_WS[n] = max(lib.cimq_lsq_quantize_workspace_bytes(n), 4)
        ws = torch.empty(nb, device=xc.device, dtype=torch.uint8)
        _lib.check(lib.cimq_lsq_quantize_backward(xc.data_ptr(), xc.numel(), sc.data_ptr(), qn, qp, scaled,
                                                  gc.data_ptr(), gx.data_ptr(), gs.data_ptr(), ws.data_ptr(),
                                                  _stream()), "cimq_lsq_quantize_backward")
        return gx, gs.reshape(ctx.s_shape), None, None, None


def lsq_quantize(x, s, qn, qp, scaled=False):
    """LSQ fake-quantiser on libcimq: round_pass(clamp(x / s, qn, qp)) [* s] (lsq.py:412,611,656)."""
    return _LsqQuantize.apply(x, s, qn, qp, scaled)


_QCONV_PLANS = {}


def _qconv_plan(*key):
    """descriptor and workspace sizes of one conv shape, built once (host time per call)"""
    p = _QCONV_PLANS.get(key)
    if p is None:
        B, C, H, W, O, KH, KW, stride, padding, dilation, code_range, has_bias = key
        desc = _lib.make_qconv_desc(B, C, H, W, O, KH, KW, stride, padding, dilation, 1, code_range[0],
                                    code_range[1], has_bias)
        p = (desc,) + tuple(_lib.qconv_sizes(desc))
        _QCONV_PLANS[key] = p
    return p


class _QConv2d(torch.autograd.Function):
    """Conv2dLSQ's quantised conv (lsq.py:436): conv2d(x_q, w_q, bias) * act_scale * w_scale with
    integer-code operands, forward on int8 MFMA (cimq_qconv_forward).  Backward: the scale
    products and grad_y0 on libcimq (cimq_qconv_backward_scales), the conv's input / weight
    gradients of grad_y0 as plain fp32 convolutions (torch.nn.grad: the library conv)."""

    @staticmethod
    def forward(ctx, x_q, act_scale, w_q, w_scale, bias, stride, padding, dilation, code_range):
        _require_device(x_q, act_scale, w_q, w_scale, bias)
        xc = x_q.detach().float().contiguous()
        wc = w_q.detach().float().contiguous()
        a = act_scale.detach().float().reshape(-1)[:1].contiguous()
        s = w_scale.detach().float().reshape(-1)[:1].contiguous()
        bc = None if bias is None else bias.detach().float().contiguous()
        B, C, H, W = xc.shape
        O, _, KH, KW = wc.shape
        desc, fws, bws = _qconv_plan(B, C, H, W, O, KH, KW, stride, padding, dilation, code_range, bc is not None)
        Ho = (H + 2 * padding[0] - dilation[0] * (KH - 1) - 1) // stride[0] + 1
        Wo = (W + 2 * padding[1] - dilation[1] * (KW - 1) - 1) // stride[1] + 1
        y = torch.empty(B, O, Ho, Wo, device=xc.device, dtype=torch.float32)
        y0 = torch.empty_like(y)
        ws = torch.empty(max(fws, 16), device=xc.device, dtype=torch.uint8)
        _lib.check(_lib.load().cimq_qconv_forward(desc, xc.data_ptr(), wc.data_ptr(), a.data_ptr(), s.data_ptr(),
                                                  None if bc is None else bc.data_ptr(), y.data_ptr(), y0.data_ptr(),
                                                  ws.data_ptr(), _stream()), "cimq_qconv_forward")
        ctx.save_for_backward(xc, wc, a, s, y0)
        ctx.desc, ctx.bws = desc, bws
        ctx.conv = (tuple(stride), tuple(padding), tuple(dilation))
        ctx.shapes = (act_scale.shape, w_scale.shape, bias is not None)
        return y

    @staticmethod
    def backward(ctx, g):
        xc, wc, a, s, y0 = ctx.saved_tensors
        stride, padding, dilation = ctx.conv
        gc = g.float().contiguous()
        gy0 = torch.empty_like(y0)
        scales = torch.empty(2, device=y0.device, dtype=torch.float32)
        ws = torch.empty(max(ctx.bws, 16), device=y0.device, dtype=torch.uint8)
        _lib.check(_lib.load().cimq_qconv_backward_scales(ctx.desc, gc.data_ptr(), y0.data_ptr(), a.data_ptr(),
                                                          s.data_ptr(), gy0.data_ptr(), scales.data_ptr(),
                                                          ws.data_ptr(), _stream()), "cimq_qconv_backward_scales")
        a_shape, s_shape, has_bias = ctx.shapes
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = torch.nn.grad.conv2d_input(xc.shape, wc, gy0, stride, padding, dilation, 1)
        if ctx.needs_input_grad[2]:
            gw = torch.nn.grad.conv2d_weight(xc, wc.shape, gy0, stride, padding, dilation, 1)
        gb = gy0.sum(dim=(0, 2, 3)) if has_bias else None
        return gx, scales[1:2].reshape(a_shape), gw, scales[0:1].reshape(s_shape), gb, None, None, None, None


def qconv2d(x_q, act_scale, w_q, w_scale, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1),
            code_range=(-128, 127)):
    """conv2d(x_q, w_q, bias) * act_scale * w_scale on int8 MFMA; x_q / w_q hold integer codes,
    x_q's within ``code_range`` (ActLSQ's [Qn, Qp]; [0, 255] runs as two 4-bit halves)."""
    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (int(v), int(v))  # noqa: E731
    return _QConv2d.apply(x_q, act_scale, w_q, w_scale, bias, pair(stride), pair(padding), pair(dilation),
                          tuple(int(c) for c in code_range))
