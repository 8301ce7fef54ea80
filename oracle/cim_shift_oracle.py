"""CPU oracle for the scale/shift ("beta") ADC variants of the CiM conv.

TEST INFRASTRUCTURE ONLY (see ``cim_oracle`` header): nothing in ``cim_quantization_amd``
imports it; ``tests/`` and ``tests/golden/make_golden.py`` use it as the checker.

The reference library's ADC has a scale only (``alpha_cim``, lsq.py:196-230).  The scale +
shift ADC lives in the test script ``test/test_backward_cimlayer_scale_shift.py`` as two
custom-autograd Functions, restated here in numpy step by step:

* ``get_analog_partial_sums_autograd_ver2`` (:336-546) -- "round" variant:
  ``adc = clamp(round((ps - beta)/alpha), Qn, Qp) * alpha + beta`` on partial sums stored in an
  int8 buffer (:401-420, truncation/wrap), STE mask from the same shifted/scaled ps (:469-484),
  ``grad_alpha = sum_{b,p} (round(ps_s) - ps_s | Qp | Qn) * G`` (:488-495, no 1/sqrt factor),
  ``grad_beta = sum_{b,p} [clamped] * G`` (:496-501).
* ``get_adcless_cim_output`` (:113-334) -- "sign" variant: ``adc = sign((ps - beta)/alpha) *
  alpha + beta`` on fp16 partial sums (:182); masks from the same quantity (:202-204);
  ``grad_alpha = sum sign * G / sqrt(numel * Qp)`` (:281-285), ``grad_beta = sum G`` (:287).

Both take integer activations / weights (no LSQ scales), slice activations unsigned
(test-local ``slicing_act`` :29-56) and weights signed (``slicing_weights`` :59-97).
The module option of this build (``Conv2dLSQCiM(adc_shift=True)``) applies the "round" ADC to
the library's rescaled partial sum instead; its oracle is ``cim_oracle.cim_forward(beta=...)``.
"""
from __future__ import annotations

import math

import numpy as np

from . import cim_oracle as co

F32 = np.float32

VARIANT_ROUND = "round"  # get_analog_partial_sums_autograd_ver2
VARIANT_SIGN = "sign"    # get_adcless_cim_output


def adc_range_shift(adc_bits):
    """Qn/Qp of the scale/shift Functions (:369-375): 2^(b-1)-1 / -2^(b-1), +-1 for 1 bit."""
    if adc_bits == 1:
        return -1.0, 1.0
    return -1.0 * (2 ** (adc_bits - 1)), (2 ** (adc_bits - 1)) - 1.0


class ShiftCtx:
    """What the scale/shift Functions keep for backward."""


def shift_forward(x_int, w_int, stride, padding, act_bits, act_bs, w_bits, w_bs, adc_bits, arr,
                  binary_mask, alpha, beta, variant=VARIANT_ROUND):
    """Forward of ver2 (:340-431) / adcless (:117-234). Returns out [B, P, O] fp32 and ctx."""
    x_int = np.asarray(x_int, F32)
    w_int = np.asarray(w_int, F32)
    nbw, nba = int(w_bits / w_bs), int(act_bits / act_bs)
    O, C, k = w_int.shape[0], w_int.shape[1], tuple(w_int.shape[2:])
    qn, qp = adc_range_shift(adc_bits)
    x_unf = co.unfold(x_int, k, padding, stride)                           # :379
    B, P, K = x_unf.shape
    xs = co.slicing_act(x_unf, act_bits, act_bs).transpose(1, 0, 2, 3)   # :383  [B, nba, P, K]
    xs = xs.astype(np.float16).astype(F32)
    ws = co.slicing_signed(w_int.reshape(O, -1).T, w_bits, w_bs)          # :392  [nbw, K, O]
    ws = ws.astype(np.float16).astype(F32)
    T = math.ceil(K / arr)
    ps = np.empty((B, T, nbw, nba, P, O), F32)
    for i, (lo, hi) in enumerate(co._tiles(K, arr)):                      # :406-418
        for j in range(nba):
            for kk in range(nbw):
                ps[:, i, kk, j] = np.matmul(xs[:, j, :, lo:hi], ws[kk, lo:hi, :]).astype(np.float16)
    if variant == VARIANT_ROUND:
        ps = co.to_int8(ps).astype(F32)                                    # :401 int8 buffer
    ctx = ShiftCtx()
    ctx.xs8 = co.to_int8(xs)                                               # :385 ctx.x_unf_sliced
    ctx.w_sliced8 = co.to_int8(ws)
    a = np.asarray(alpha, F32)
    b = np.asarray(beta, F32)
    u = ps
    with np.errstate(all="ignore"):
        ps_s = ((u - b).astype(F32) / a).astype(F32)                       # :421 / :202
        if variant == VARIANT_ROUND:
            code = np.clip(np.rint(ps_s), F32(qn), F32(qp)).astype(F32)     # :424
        else:
            code = np.sign(ps_s).astype(F32)                                # :209
        adc = ((code * a).astype(F32) + b).astype(F32)                     # :425 / :211
    out = np.sum((adc * np.asarray(binary_mask, F32)).astype(F32), axis=(1, 2, 3), dtype=F32)  # :429 / :215
    ctx.ps_s, ctx.code = ps_s, code
    ctx.meta = dict(stride=tuple(stride), padding=tuple(padding), k=k, C=C, O=O, H=x_int.shape[2],
                    W=x_int.shape[3], nbw=nbw, nba=nba, w_bs=w_bs, act_bs=act_bs, arr=arr, T=T, K=K, P=P,
                    B=B, qn=qn, qp=qp, variant=variant)
    ctx.binary_mask = np.asarray(binary_mask, F32)
    return out.astype(F32), ctx


def shift_backward(ctx: ShiftCtx, grad_out, absolute=False):
    """Backward of ver2 (:437-546) / adcless (:240-334): (gx, gw, grad_alpha, grad_beta).

    ``absolute`` re-runs every contraction in fp64 on |operands| (the per-element sum of
    |terms| that the parity tolerances scale by)."""
    m = ctx.meta
    dt = np.float64 if absolute else F32
    A = (np.abs if absolute else (lambda v: v))
    nbw, nba, T, K, P, B, O = m["nbw"], m["nba"], m["T"], m["K"], m["P"], m["B"], m["O"]
    qn, qp = m["qn"], m["qp"]
    w_sl = ctx.w_sliced8.astype(dt)                                         # :441
    xs = ctx.xs8.astype(dt)                                                 # :438, ctx.x_unf_sliced of :385
    g = np.asarray(grad_out, dt)
    G = np.broadcast_to(g[:, None, None, None], (B, T, nbw, nba, P, O))    # :472-476
    G = (G * ctx.binary_mask.astype(dt)).astype(dt)                         # :478
    ps_s = ctx.ps_s
    with np.errstate(invalid="ignore"):
        ge = ps_s >= F32(qp + 1e-5)
        le = ps_s <= F32(qn - 1e-5)
    clamped = ge | le
    Gm = np.where(clamped, dt(0), G).astype(dt)                             # :484 / :277
    if m["variant"] == VARIANT_ROUND:
        with np.errstate(invalid="ignore"):
            q = (np.rint(ps_s) - ps_s).astype(F32).astype(dt)               # :488
        q = np.where(ge, dt(qp), q)
        q = np.where(le, dt(qn), q)
        ga = np.sum((A(q) * A(G)).astype(dt), axis=(0, 4), keepdims=True)  # :489-495
        gb = np.sum(np.where(clamped, A(G), dt(0)), axis=(0, 4), keepdims=True)  # :496-501
    else:
        c = F32(1.0 / math.sqrt(ps_s.size * qp)) if not absolute else 1.0 / math.sqrt(ps_s.size * qp)
        ga = np.sum(((A(ctx.code.astype(dt)) * A(G)).astype(dt) * dt(c)).astype(dt), axis=(0, 4), keepdims=True)
        gb = np.sum(A(G), axis=(0, 4), keepdims=True)                        # :287
    gi = np.zeros((B, nbw, nba, P, K), dt)
    gw = np.zeros((nbw, nba, K, O), dt)
    for i, (lo, hi) in enumerate(co._tiles(K, m["arr"])):                   # :504-521
        for j in range(nba):
            xt = A(xs[:, j, :, lo:hi]).transpose(0, 2, 1)
            for kk in range(nbw):
                gt = A(Gm[:, i, kk, j])
                gi[:, kk, j, :, lo:hi] = np.matmul(gt, A(w_sl[kk, lo:hi, :]).T)
                gw[kk, j, lo:hi, :] = np.matmul(xt, gt).sum(0)
    gw = gw.sum(axis=1)                                                     # :520-525
    for i in range(1, nbw):
        gw[i] = gw[i] / dt((2 ** m["w_bs"]) ** i)
    gw = gw.mean(axis=0, dtype=dt)                                          # :527
    gw = np.ascontiguousarray(gw.T).reshape(O, m["C"], *m["k"])            # :530
    gi = gi.sum(axis=1)                                                     # :533
    for i in range(1, nbw):                                                 # :534-535 (bound nbw)
        gi[:, i] = gi[:, i] / dt((2 ** m["act_bs"]) ** i)
    gi = gi.mean(axis=1, dtype=dt)                                          # :537
    gx = co.fold(gi.transpose(0, 2, 1), (m["H"], m["W"]), m["k"], m["padding"], m["stride"])  # :540-542
    return gx.astype(dt), gw.astype(dt), ga.astype(dt), gb.astype(dt)
