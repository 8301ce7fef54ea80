/*
 * cimq.h -- C ABI of libcimq.so, the MI355X (gfx950) implementation of the CiM
 * partial-sum-quantised convolution of UtkarshSaxena1/CiM_Quantization.
 *
 * The reference path is pure PyTorch (models/_modules/lsq.py); its device work is
 * stock torch ops issued from Python.  libcimq replaces that device work with
 * hand-written CDNA4 HIP kernels.  The Python host layer (cim_quantization_amd)
 * binds these symbols with ctypes; any other FFI (cgo, JNI, N-API) can bind them the
 * same way.
 *
 * Conventions
 *  - Every pointer argument is DEVICE memory owned by the caller (e.g. a torch
 *    tensor's data_ptr()).  The library allocates nothing; scratch comes from the
 *    caller's ``ws`` of cimq_query_sizes()->*_workspace_bytes.
 *  - Scalars that live on the device in the reference (the LSQ step sizes sw/sa,
 *    alpha_cim, signed_act) are passed as device pointers: no host synchronisation.
 *  - All launches are stream-ordered on ``stream`` (a hipStream_t, passed as void*;
 *    NULL = the legacy default stream).  Functions are reentrant and keep no global
 *    mutable state apart from a thread-local error string.
 *  - Return value: 0 on success, otherwise a CIMQ_E* code; cimq_last_error() gives
 *    the message.  Nothing throws across the ABI.
 *
 * Tensor layouts (identical to the reference):
 *   x, grad_x      [B, C, H, W]              fp32, NCHW contiguous
 *   w_q, grad_w    [O, C, KH, KW]            fp32
 *   out, grad_out  [B, Ho*Wo, O]             fp32 (the Function's [B, P, O] output)
 *   alpha_q        [1, T, nbw, nba, 1, O]    fp32 (quantised alpha_cim), may be NULL
 *   binary_mask    [1, 1, nbw, nba, 1, 1]    int8 (wraps for 8-bit layers)
 *   signed_act     [1]                       fp32 buffer (0 or 1)
 */
#ifndef CIMQ_H
#define CIMQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CIMQ_ABI_VERSION 16
/* additions that change no existing struct or call: 1 = activation codes (cimq_act_codes,
 * cimq_module_forward_codes, cimq_module_codes_supported) */
#define CIMQ_ABI_MINOR 1

/* status codes */
#define CIMQ_OK 0
#define CIMQ_EINVAL 1      /* descriptor / argument rejected */
#define CIMQ_EUNSUPPORTED 2 /* valid for the reference but not implemented here */
#define CIMQ_EHIP 3        /* a HIP runtime call failed */

/* what ``x`` holds (cimq_conv_desc.input_kind) */
#define CIMQ_INPUT_XQ 0     /* x is x_q, the quantised activation handed to the Function (lsq.py:92) */
#define CIMQ_INPUT_RAW_LSQ 1 /* x is the raw activation; the LSQ act quantiser (lsq.py:547-549) is fused */

/* cimq_conv_desc.adc_variant: which ADC the partial sums go through.  Low byte = variant,
 * higher bits = CIMQ_ADC_F_* modifiers. */
#define CIMQ_ADC_LIBRARY 0     /* get_cim_output_signed's ADC (lsq.py:196-230), deterministic */
#define CIMQ_ADC_STOCHASTIC 1  /* the stochastic 1.5-bit ADC (lsq.py:205-221): 2 x 50 Bernoulli draws
                                  per partial sum from a Philox4x32-10 stream keyed by seed_lo/hi;
                                  the backward is the deterministic one (lsq.py:244-386) */
#define CIMQ_ADC_SHIFT_ROUND 2 /* scale + shift ADC clamp(round((u-beta)/alpha))*alpha + beta
                                  (test/test_backward_cimlayer_scale_shift.py:336-546, "ver2") */
#define CIMQ_ADC_SHIFT_SIGN 3  /* scale + shift sign ADC sign((u-beta)/alpha)*alpha + beta
                                  (test/test_backward_cimlayer_scale_shift.py:113-334, "adcless") */
#define CIMQ_ADC_F_PS_INT8 0x100     /* partial sums pass through an int8 buffer before the ADC
                                        (truncation + wrap, scale_shift.py:401) */
#define CIMQ_ADC_F_SHIFT_RANGE 0x200 /* ADC range Qp = 2^(b-1)-1, Qn = -2^(b-1) for every adc_bits
                                        but 1 (scale_shift.py:369-375) instead of the library's
                                        +-1 for 1.5 bits */

/* cimq_conv_desc.options */
#define CIMQ_OPT_RECOMPUTE 1 /* module entry points: where a recompute backward exists (CIMQ_ROUTE_R6: w3a3 16 -> 16,
                                3x3 stride 1, xbar 128, 32 wide) the forward writes no per-partial-sum state words
                                and the backward recomputes the partial sums -- a smaller ctx (module_ctx_bytes;
                                33.5 MB less per such layer at B = 256) for a slower backward on MI355X (DESIGN.md
                                section 10).  Ignored elsewhere.  Since ABI 14 */
/* (bit value 2 is not an option: descriptors carrying it are refused) */
#define CIMQ_OPT_INFERENCE 4 /* forward only (evaluation under no-grad): cimq_forward, cimq_module_forward,
                                cimq_module_shift_forward and cimq_module_prepare compute ``out`` bit for bit as
                                without it -- same kernels, same summation order, same Philox draws -- and write
                                nothing a backward would read: no state words, no backward activation words, none
                                of the backward-only weight operands.  cimq_query_sizes then reports ctx_bytes ==
                                module_ctx_bytes (the weight-side tables, plus the forward slice words on the routes
                                whose forward does not quantise the activation itself), bwd_workspace_bytes == 0
                                and a fwd_workspace_bytes of forward scratch only; wprep_bytes is unchanged, and a
                                wprep buffer must be made with the descriptor it is used with.  cimq_module_route
                                reports CIMQ_ROUTE_NONE for both backward roles.  Every other entry point that takes
                                a cimq_conv_desc refuses the bit with CIMQ_EINVAL.  CIMQ_OPT_RECOMPUTE may be set
                                with it and then has no effect.  Since ABI 15 */

/* cimq_lsq_desc.flags */
#define CIMQ_LSQ_ACCUMULATE_GRADS 1 /* cimq_module_backward adds the parameter gradients into
                                       grad_weight / grad_alpha_* (torch's AccumulateGrad,
                                       grad = grad + new) instead of overwriting them */
#define CIMQ_LSQ_SKIP_TAIL 2        /* cimq_module_backward stops after grad_x and the per-chunk
                                       grad_w / grad_alpha partials (left in ws); the caller runs
                                       cimq_module_backward_tail later, e.g. on a second stream
                                       (the parameter gradients are off the grad_x chain) */
#define CIMQ_LSQ_DEFER_GW 4         /* as SKIP_TAIL, and on layers whose grad_w is a kernel of its
                                       own (the v7 pair) that kernel is left out too: the caller
                                       runs cimq_module_backward_params (grad_w + the epilogue) on
                                       a second stream ordered after cimq_module_backward.  Since ABI 10 */

typedef struct cimq_conv_desc {
  int32_t batch, in_channels, in_h, in_w; /* B, C, H, W */
  int32_t out_channels, kernel_h, kernel_w; /* O, KH, KW (square kernels in the reference) */
  int32_t stride_h, stride_w, pad_h, pad_w;
  int32_t xbar;       /* crossbar rows per tile ("arr", lsq.py:166); multiple of 16 */
  int32_t bits_w, bits_a; /* nbits_w, nbits_a */
  int32_t bs_w, bs_a; /* weight / activation bit-slice widths */
  float adc_bits;     /* 0 (fp ADC), 1 (sign), 1.5 (ternary, alpha scaled), >1.5 (multi-level) */
  int32_t input_kind; /* CIMQ_INPUT_* */
  float lsq_qp;       /* CIMQ_INPUT_RAW_LSQ: act clamp max Qp_a = 2^bits_a - 1 (Qn_a = 0) */
  int32_t adc_variant; /* CIMQ_ADC_* | CIMQ_ADC_F_* (0: the library ADC) */
  uint32_t seed_lo, seed_hi; /* CIMQ_ADC_STOCHASTIC: Philox key of this call */
  int32_t options;    /* CIMQ_OPT_* bits (0: the defaults); was ``reserved`` before ABI 14 */
} cimq_conv_desc;

/* The LSQ quantisers of Conv2dLSQCiM.forward (lsq.py:544-571), for the module entry points. */
typedef struct cimq_lsq_desc {
  float qn_w, qp_w;         /* weight clamp range: -2^(bits_w-1), 2^(bits_w-1)-1 (lsq.py:553-555) */
  float gscale_a;           /* grad_scale factor of alpha_act: 1/sqrt(numel(x) * Qp_a) (lsq.py:547) */
  float gscale_w;           /* grad_scale factor of alpha_weight: 1/sqrt(numel(w) * Qp_w) (lsq.py:553) */
  int32_t nbits_alpha;      /* alpha_cim quantiser bits (lsq.py:566-571); ignored unless adc 1 / 1.5 */
  int32_t flags;            /* CIMQ_LSQ_* bits */
  const void* wprep;        /* NULL, or a buffer of cimq_sizes.wprep_bytes that cimq_module_prepare
                               filled for this descriptor pair and the current parameter values:
                               the module forward then runs only the activation quantiser, and it
                               and the backward read the weight-side state (w_q operands, alpha_q
                               thresholds, step sizes) from there instead of from ctx */
} cimq_lsq_desc;

typedef struct cimq_sizes {
  size_t ctx_bytes;           /* forward -> backward state, caller-owned device memory */
  size_t fwd_workspace_bytes; /* scratch for cimq_forward / cimq_alpha_init */
  size_t bwd_workspace_bytes; /* scratch for cimq_backward */
  size_t wprep_bytes;         /* weight-side state of the module entry points (cimq_module_prepare) */
  size_t module_ctx_bytes;    /* ctx of the module entry points (cimq_module_forward / _backward): smaller than
                                 ctx_bytes where their backward recomputes the partial sums instead of reading
                                 per-partial-sum state words (CIMQ_ROUTE_R6 under CIMQ_OPT_RECOMPUTE).  Since ABI 13 */
} cimq_sizes;

/* ABI version of the loaded library (compare with CIMQ_ABI_VERSION). */
int cimq_abi_version(void);
/* ... and its CIMQ_ABI_MINOR (a library from before the first addition has no such symbol). */
int cimq_abi_minor(void);

/* Message of the last failing call on this thread ("" if none). */
const char* cimq_last_error(void);

/* Validate a descriptor and report the buffer sizes it needs.
 * Replaces the geometry bookkeeping of get_cim_output_signed.forward (lsq.py:115-170). */
int cimq_query_sizes(const cimq_conv_desc* d, cimq_sizes* out);

/* Forward of the CiM conv: act codes + bit slices, implicit-im2col int8 MFMA partial sums
 * per (tile, w-slice, a-slice), ADC requantisation and shift-and-add.
 * Replaces get_cim_output_signed.forward (lsq.py:92-237); with CIMQ_INPUT_RAW_LSQ it
 * also absorbs the activation quantiser of Conv2dLSQCiM.forward (lsq.py:547-549).
 * out = [B, P, O]; ctx receives what cimq_backward needs (the int8 ctx of lsq.py:99,160
 * and the parameters that stand in for the fp16 partial sums of lsq.py:192). */
int cimq_forward(const cimq_conv_desc* d, const float* x, const float* w_q, const float* sa,
                 const float* sw, const float* alpha_q, const int8_t* binary_mask,
                 const float* signed_act, float* out, void* ctx, void* ws, void* stream);

/* Backward of the CiM conv.  Replaces get_cim_output_signed.backward (lsq.py:244-386):
 *   grad_x     [B,C,H,W]  d loss / d x_q (CIMQ_INPUT_XQ) or d loss / d x through the
 *                          fused LSQ quantiser (CIMQ_INPUT_RAW_LSQ)
 *   grad_w     [O,C,KH,KW] d loss / d w_q
 *   grad_alpha [1,T,nbw,nba,1,O] d loss / d alpha_q (adc 1 / 1.5 only, else may be NULL)
 *   grad_sa    [1]  CIMQ_INPUT_RAW_LSQ only: d loss / d sa from the LSQ graph (lsq.py:548-549)
 * ``x``, ``sa``, ``sw``, ``alpha_q``, ``binary_mask``, ``signed_act`` must be the same
 * buffers (same contents) that were given to cimq_forward with this ctx. */
int cimq_backward(const cimq_conv_desc* d, const float* grad_out, const float* x, const float* sa,
                  const float* sw, const float* alpha_q, const int8_t* binary_mask,
                  const float* signed_act, const void* ctx, float* grad_x, float* grad_w,
                  float* grad_alpha, float* grad_sa, void* ws, void* stream);

/* Forward of a whole Conv2dLSQCiM layer after its first-step initialisation (lsq.py:544-581):
 * the activation, weight and alpha_cim quantisers run inside the library on the raw
 * parameters, then the CiM conv; ``out`` is the module's NCHW output [B, O, Ho, Wo] (before
 * the optional bias).  Requires input_kind = CIMQ_INPUT_RAW_LSQ.  ``alpha_cim`` may be NULL
 * unless adc_bits is 1 or 1.5.  ``ctx`` must hold cimq_query_sizes()->module_ctx_bytes (ABI 13; ctx_bytes
 * is never smaller) and ``ws`` fwd_workspace_bytes. */
int cimq_module_forward(const cimq_conv_desc* d, const cimq_lsq_desc* q, const float* x, const float* weight,
                        const float* alpha_act, const float* alpha_weight, const float* alpha_cim,
                        const int8_t* binary_mask, const float* signed_act, float* out, void* ctx, void* ws,
                        void* stream);

/* Backward of cimq_module_forward: from d loss / d out (NCHW) to the gradients of the raw
 * activation and of the four parameters (weight, alpha_act, alpha_weight, alpha_cim), through
 * the quantisers as torch's autograd differentiates them.  With CIMQ_LSQ_ACCUMULATE_GRADS in
 * q->flags the parameter gradients are added into the four grad buffers (grad_x is always
 * overwritten).  ctx must come from cimq_module_forward. */
int cimq_module_backward(const cimq_conv_desc* d, const cimq_lsq_desc* q, const float* grad_out, const float* x,
                         const float* weight, const float* alpha_act, const float* alpha_weight,
                         const float* alpha_cim, const int8_t* binary_mask, const float* signed_act,
                         const void* ctx, float* grad_x, float* grad_weight, float* grad_alpha_act,
                         float* grad_alpha_weight, float* grad_alpha_cim, void* ws, void* stream);

/* The parameter-gradient epilogue of cimq_module_backward (slab reductions of grad_w and
 * grad_alpha, the weight / alpha_cim quantiser backward, the two step-size gradients) for a
 * backward run with CIMQ_LSQ_SKIP_TAIL: ``ctx`` and ``ws`` are that call's, unchanged, and the
 * stream must be ordered after it.  Replaces the torch autograd of lsq.py:547-571 into the
 * parameters.  q->flags as that call's (CIMQ_LSQ_ACCUMULATE_GRADS honoured). */
int cimq_module_backward_tail(const cimq_conv_desc* d, const cimq_lsq_desc* q, const float* weight,
                              const float* alpha_cim, const void* ctx, float* grad_weight, float* grad_alpha_act,
                              float* grad_alpha_weight, float* grad_alpha_cim, void* ws, void* stream);

/* The parameter-gradient half of a cimq_module_backward run with CIMQ_LSQ_DEFER_GW: the grad_w
 * kernel that call left out (if the layer has one of its own), then the epilogue of
 * cimq_module_backward_tail.  grad_out, ctx and ws are that call's, unchanged; the stream must be
 * ordered after it (grad_w reads only grad_out and the forward's state, so it overlaps the next
 * layer's grad_x when it runs on a second stream).  q->flags as that call's.  Since ABI 10. */
int cimq_module_backward_params(const cimq_conv_desc* d, const cimq_lsq_desc* q, const float* grad_out,
                                const float* weight, const float* alpha_cim, const void* ctx, float* grad_weight,
                                float* grad_alpha_act, float* grad_alpha_weight, float* grad_alpha_cim, void* ws,
                                void* stream);

/* cimq_module_forward / cimq_module_backward for Conv2dLSQCiM(adc_shift=True): the per-tile scale +
 * shift ADC clamp(round((u - beta) / alpha_q), -1, 1) * alpha_q + beta of
 * test/test_backward_cimlayer_scale_shift.py:336-546 applied to the library's rescaled partial sum
 * u = fp16(ps) * sw * sa, with the three quantisers inside the library as for the library ADC.
 * Requires adc_variant = CIMQ_ADC_SHIFT_ROUND (no flags), adc_bits 1.5, input_kind =
 * CIMQ_INPUT_RAW_LSQ, nbw = nba = 2 or 3 and a layer the fast path takes (3x3, pad 1, stride 1 or 2,
 * power-of-two output width and channels); CIMQ_EUNSUPPORTED otherwise (the caller then quantises
 * in torch and calls cimq_shift_forward / cimq_shift_backward).  A prepared weight side (q->wprep, made
 * by cimq_module_prepare_shift) with a CIMQ_OPT_INFERENCE descriptor only: the backward reads nothing
 * prepared, so a training descriptor with q->wprep set is CIMQ_EINVAL.  No CIMQ_LSQ_SKIP_TAIL.
 * beta_cim / grad_beta_cim: [1, T, nbw, nba, 1, O] like alpha_cim; CIMQ_LSQ_ACCUMULATE_GRADS adds into
 * grad_beta_cim as well.  Since ABI 8. */
int cimq_module_shift_supported(const cimq_conv_desc* d); /* 1 if the two calls below take d, else 0 */

/* Which kernels cimq_module_forward / cimq_module_backward run for d (the library ADC, the module entry
 * points): route[0] forward, route[1] grad_x, route[2] grad_w (+ grad_alpha_cim partials), each one of
 * the CIMQ_ROUTE_* codes below.  Pure host query, no device work.  Returns 0, or an error status for a
 * descriptor the module entry points refuse.  Since ABI 12. */
enum {
  CIMQ_ROUTE_GENERAL = 0,  /* the general kernels */
  CIMQ_ROUTE_V3 = 1,       /* forward: cim_fwd_v3_kernel */
  CIMQ_ROUTE_FWD5 = 2,     /* forward: cim_fwd5_kernel (slice-planar patch, round 5) */
  CIMQ_ROUTE_V7 = 3,       /* grad_x: cim_bwd_gx_v8_kernel / grad_w: cim_bwd_gw_v7_kernel */
  CIMQ_ROUTE_FUSED = 4,    /* grad_x and grad_w in cim_bwd_fused_kernel */
  CIMQ_ROUTE_C1 = 5,       /* the w8a8 first conv: cim_bwd_c1_kernel (both) */
  CIMQ_ROUTE_GX5 = 6,      /* grad_x: cim_bwd_gx5_kernel (per input pixel, round 5) */
  CIMQ_ROUTE_GW5 = 7,      /* grad_w: cim_bwd_gw5_kernel (A-ready patch, round 5) */
  CIMQ_ROUTE_DENSE = 8,    /* the dense 1x1 path */
  CIMQ_ROUTE_R6 = 9,       /* grad_x and grad_w in cim_bwd_r6_kernel from RECOMPUTED partial sums (the forward
                              writes no state words; round 6, ABI 13; only under CIMQ_OPT_RECOMPUTE since ABI 14) */
  CIMQ_ROUTE_NONE = 10,    /* route[1] / route[2] under CIMQ_OPT_INFERENCE: there is no backward.  Since ABI 15 */
  CIMQ_ROUTE_WIDE = 11     /* forward: cim_fwd_wide_kernel, the channel-chunked forward of 3x3 module layers from 128
                              input channels up (cimq_wide_abi() == 1); their backward stays CIMQ_ROUTE_GENERAL */
};
int cimq_module_route(const cimq_conv_desc* d, int* route);

/* 1 where forward-only w4a4 layers in 1-bit slices (four slices a side, the library ADC) run the stateless word-pair
 * forward -- one launch per prepared layer, the activation quantised in the kernel's row staging -- and
 * cimq_module_forward_form exists (a library from before them has neither symbol).  CIMQ_ABI_VERSION / _MINOR and
 * cimq_net_abi() are unchanged: no struct, call, size or route name moved. */
int cimq_w4a4_eval_abi(void);

/* Which form of the forward kernel family the module entry points run for `d`.  Pure host query, no device work.
 *   form[0]  the family's state format: 0 the per-k words, 2 / 3 the compact words of w2a2 / w3a3, 4 the word pairs
 *            of w4a4 in 1-bit slices, 8 the w8a8 planes.  Under CIMQ_OPT_INFERENCE no words are written; the number
 *            still names the kernel form (4: on every shape whose training call runs that format).
 *   form[1]  1 where the module forward quantises the activation in its own row staging, so that a call whose
 *            weight side is prepared (q->wprep) is one launch with no pass over x before it; else 0.
 * Returns 0, CIMQ_EINVAL for a NULL argument, or the status of a descriptor the module entry points refuse. */
int cimq_module_forward_form(const cimq_conv_desc* d, int form[2]);

/* 1 where module layers whose input channels do not fit the fast forward's whole-C LDS patch (C >= 128, C and O
 * multiples of 16, the fast path's pixel geometry, the library ADC, at most four slices a side) run
 * cim_fwd_wide_kernel: route[0] is CIMQ_ROUTE_WIDE, the training forward writes NCHW in one launch after the
 * prologue, and a prepared forward-only layer -- plain or with an epilogue -- is one launch.  The route takes no
 * activation codes and no residual view: cimq_module_codes_supported answers 0 / 0, and cimq_module_forward_codes /
 * cimq_net_forward return CIMQ_EUNSUPPORTED before any launch.  Every size (cimq_query_sizes, cimq_sizes) is what it
 * was: the [B, P, O] workspace region and a forward-only call's slice-word region simply go unwritten.
 * CIMQ_ABI_VERSION / _MINOR and the other availability numbers are unchanged. */
int cimq_wide_abi(void);

/* The plan of that forward for `d`, without device work: out[0] 1 where the route applies (else 0, and the rest 0),
 * out[1] the channel chunks the LDS patch is staged in per 64-pixel m-tile, out[2] the output groups of up to four
 * 16-channel blocks (the grid's y), out[3] the crossbar tiles.  Returns 0, CIMQ_EINVAL for a NULL argument, or the
 * status of a descriptor the module entry points refuse. */
int cimq_module_wide_plan(const cimq_conv_desc* d, int out[4]);
int cimq_module_shift_forward(const cimq_conv_desc* d, const cimq_lsq_desc* q, const float* x, const float* weight,
                              const float* alpha_act, const float* alpha_weight, const float* alpha_cim,
                              const float* beta_cim, const int8_t* binary_mask, const float* signed_act, float* out,
                              void* ctx, void* ws, void* stream);
int cimq_module_shift_backward(const cimq_conv_desc* d, const cimq_lsq_desc* q, const float* grad_out,
                               const float* x, const float* weight, const float* alpha_act,
                               const float* alpha_weight, const float* alpha_cim, const float* beta_cim,
                               const int8_t* binary_mask, const float* signed_act, const void* ctx, float* grad_x,
                               float* grad_weight, float* grad_alpha_act, float* grad_alpha_weight,
                               float* grad_alpha_cim, float* grad_beta_cim, void* ws, void* stream);

/* cimq_epilogue.flags */
#define CIMQ_EPI_RELU 1 /* y = (y < 0) ? 0 : y as the last step (a NaN stays NaN) */

/* The output epilogue of cimq_module_forward_epilogue: per output channel o, with v the value
 * cimq_module_forward stores at (b, o, h, w),
 *   y = v * scale[o];  y = y + shift[o];  y = y + residual[b, o, h, w] (residual != NULL);  ReLU (CIMQ_EPI_RELU)
 * each step one IEEE fp32 operation, in that order, no fused multiply-add: what torch's mul, add, add, relu give
 * on the stored tensor.  A BatchNorm in evaluation mode folds into (scale, shift).  Since ABI 16. */
typedef struct cimq_epilogue {
  const float* scale;    /* [O] device */
  const float* shift;    /* [O] device */
  const float* residual; /* NULL, or [B, O, Ho, Wo] NCHW fp32, 16-byte aligned, not overlapping out */
  int32_t flags;         /* CIMQ_EPI_* */
  int32_t reserved;      /* 0 */
} cimq_epilogue;

/* cimq_module_forward (beta_cim NULL) or cimq_module_shift_forward (beta_cim given, by that call's rules) of a
 * CIMQ_OPT_INFERENCE descriptor with ``epi`` applied in the registers of the kernel that stores ``out``: the same
 * launches, the same buffers (cimq_query_sizes; no extra workspace), the same q->wprep rules, and ``out`` equal
 * bit for bit to the epilogue's four operations run on cimq_module_forward's output.  CIMQ_EINVAL for a
 * descriptor without CIMQ_OPT_INFERENCE, a NULL epi / scale / shift, unknown flag bits, a non-zero reserved, a
 * residual that is not 16-byte aligned or that overlaps out.  Since ABI 16. */
int cimq_module_forward_epilogue(const cimq_conv_desc* d, const cimq_lsq_desc* q, const float* x,
                                 const float* weight, const float* alpha_act, const float* alpha_weight,
                                 const float* alpha_cim, const float* beta_cim, const int8_t* binary_mask,
                                 const float* signed_act, const cimq_epilogue* epi, float* out, void* ctx, void* ws,
                                 void* stream);

/* ---- the epilogue's values through a 2x2 max pool (cimq_pool_abi() == 1; CIMQ_ABI_VERSION / _MINOR and the other
 * availability numbers are unchanged: new symbols alone) ----
 *
 * A CIMQ_ROUTE_WIDE layer can store, instead of its [B, O, Ho, Wo] output, that output's 2x2 / stride-2 max pool
 * [B, O, Ho/2, Wo/2], computed in the registers of the storing kernel on the values the epilogue produces (scale,
 * shift, residual, ReLU): bit for bit torch's max_pool2d(., 2, 2) of cimq_module_forward_epilogue's output -- the
 * first maximal element of a window in the order (0,0), (0,1), (1,0), (1,1), any NaN in a window gives NaN. */
#define CIMQ_POOL_MAX2 2 /* the `pool` argument / cimq_net_ext.pool entry: 2x2 windows, stride 2, no padding */

/* 1 where the calls of this section exist (a library from before them has no such symbol). */
int cimq_pool_abi(void);

/* Whether cimq_module_forward_pool takes d with pool == CIMQ_POOL_MAX2: a host query, no device work.  *ok is 1
 * where d has CIMQ_OPT_INFERENCE, its forward route is CIMQ_ROUTE_WIDE, its output is at most 32 wide (both rows of a
 * window then sit in one 64-pixel tile) and the kernel's LDS holds the row exchange (every layer of two or more weight
 * slices or two K-steps); else 0.  Returns CIMQ_OK, CIMQ_EINVAL for a NULL argument, or the descriptor's own error. */
int cimq_module_pool_supported(const cimq_conv_desc* d, int* ok);

/* cimq_module_forward_epilogue with ``pool`` before ``out``.  pool == 0: that call exactly.  pool == CIMQ_POOL_MAX2:
 * out is [B, O, Ho/2, Wo/2], the pooled plane alone is written; epi->residual keeps the unpooled shape
 * [B, O, Ho, Wo]; the same launches (one for a prepared layer), the same q->wprep rules, ctx and workspace as
 * cimq_query_sizes reports.  CIMQ_EINVAL: every refusal of cimq_module_forward_epilogue (the overlap test takes out's
 * pooled extent), any other ``pool``.  CIMQ_EUNSUPPORTED, nothing launched or written: a layer for which
 * cimq_module_pool_supported answers 0, or beta_cim given (cimq_last_error names the reason). */
int cimq_module_forward_pool(const cimq_conv_desc* d, const cimq_lsq_desc* q, const float* x, const float* weight,
                             const float* alpha_act, const float* alpha_weight, const float* alpha_cim,
                             const float* beta_cim, const int8_t* binary_mask, const float* signed_act,
                             const cimq_epilogue* epi, int pool, float* out, void* ctx, void* ws, void* stream);

/* cimq_act_codes.flags */
#define CIMQ_CODES_NO_FLOAT 1 /* out is not written and may be NULL (needs out_codes) */

/* Activations as codes between two convs.  The code of a value y entering a layer with step-size parameter
 * alpha_act, gradient-scale factor gscale_a and clamp maximum Qp (an integer in [1, 254]) is
 *   sa = (alpha_act - alpha_act * gscale_a) + alpha_act * gscale_a      (fp32, the module prologue's expression)
 *   code(y) = isnan(y) ? Qp + 1 : (uint8) rint(clamp(y / sa, 0, Qp))    (an IEEE fp32 division)
 * exactly the chain of that layer's own activation quantiser, so its slice words depend on y through code(y)
 * alone.  Layout: one byte per element, [B, C, H, W] contiguous, base 16-byte aligned. */
typedef struct cimq_act_codes {
  const uint8_t* x_codes;     /* NULL, or the input as codes (for this layer: d->lsq_qp is its Qp); x is then
                                 ignored and may be NULL.  A byte above Qp + 1 is read as Qp + 1 */
  uint8_t* out_codes;         /* NULL, or where the output's codes go, [B, O, Ho, Wo] */
  const float* out_alpha_act; /* device [1]: the consumer's alpha_act */
  float out_gscale_a;         /* the consumer's gradient-scale factor */
  float out_qp;               /* the consumer's clamp maximum */
  int32_t flags;              /* CIMQ_CODES_* */
  int32_t reserved;           /* 0 */
} cimq_act_codes;

/* Whether cimq_module_forward_codes takes descriptor d with x_codes (*in_ok) and with out_codes (*out_ok): a host
 * query, no device work.  in_ok: every forward route, where d->lsq_qp is an integer in [1, 254].  out_ok: the
 * fwd5, v3 and general forward routes (cimq_module_route); the dense kernels write no codes.  Either pointer may
 * be NULL.  Returns CIMQ_OK or the descriptor's own error. */
int cimq_module_codes_supported(const cimq_conv_desc* d, int* in_ok, int* out_ok);

/* cimq_module_forward_epilogue with the input read as codes, the output written as codes for the next layer, or
 * both (io; the other arguments are that call's, epi required -- the identity is scale 1, shift 0).  With
 * io->x_codes == NULL && io->out_codes == NULL it is cimq_module_forward_epilogue.
 *  - x_codes: ``out`` is bit for bit what the same call gives on any fp32 x whose codes these are.  Where the
 *    forward quantises in its own staging (fwd5, and v3 with the fused quantiser) the staging reads the bytes
 *    straight into its word table; on the other routes a code-reading form of the forward-only prologue writes the
 *    slice words and the forward kernels run unchanged.
 *  - out_codes[b, o, h, w] = code(y) for the consumer layer (out_alpha_act, out_gscale_a, out_qp), y the value the
 *    epilogue stores, or with CIMQ_CODES_NO_FLOAT would store, at out[b, o, h, w]: computed in the registers of
 *    the storing kernel.
 * No extra workspace (cimq_query_sizes).  CIMQ_EINVAL: every refusal of cimq_module_forward_epilogue, a NULL io, a
 * non-zero reserved or unknown flags, CIMQ_CODES_NO_FLOAT without out_codes, out_codes with a NULL out_alpha_act
 * or an out_qp that is not an integer in [1, 254], a code buffer that is not 16-byte aligned, out_codes
 * overlapping out, x_codes, x or the residual.  CIMQ_EUNSUPPORTED: x_codes for a layer whose lsq_qp is not an
 * integer in [1, 254], out_codes on the dense route (cimq_module_codes_supported).  Since ABI 16, minor 1. */
int cimq_module_forward_codes(const cimq_conv_desc* d, const cimq_lsq_desc* q, const cimq_act_codes* io,
                              const float* x, const float* weight, const float* alpha_act,
                              const float* alpha_weight, const float* alpha_cim, const float* beta_cim,
                              const int8_t* binary_mask, const float* signed_act, const cimq_epilogue* epi,
                              float* out, void* ctx, void* ws, void* stream);

/* ---- a whole fused evaluation network in one call (cimq_net_abi() == 1; CIMQ_ABI_VERSION / _MINOR unchanged) ----
 *
 * A plan is a list of conv layers that run in order on one stream, the activation slots they read and write, and an
 * optional head (global average pool + classifier).  Layer i is exactly the cimq_module_forward_codes call with these
 * arguments (cimq_module_forward_epilogue for a float-only edge): the same code path, and every float plane and code
 * plane it writes is bit for bit what that call writes.  A slot is a pair of caller-owned device buffers: a float
 * plane ([B, O, Ho, Wo] fp32) and a code plane (one byte per element), each 16-byte aligned and as large as
 * cimq_net_sizes reports; a slot may be reused once its last reader has run.
 *
 * The residual is a whole tensor of the output's shape, or a view of a larger one (ResNet's option-A shortcut,
 * F.pad(src[:, :, ::s, ::s], channels)): with the source [B, Cr, Hr, Wr] in res_slot, out (b, o, h, w) adds
 * src[b, o - res_c0, s h, s w] where res_c0 <= o < res_c0 + Cr and +0.0f elsewhere (a real add: -0.0 becomes +0.0),
 * read in the epilogue of the kernel that stores the output -- bit for bit the add of the materialised tensor. */
#define CIMQ_NET_HEAD_MAX_C 8192 /* cimq_net_head: the pooled features of one image live in LDS (32 KB) */

typedef struct cimq_net_layer {
  const cimq_conv_desc* desc; /* CIMQ_OPT_INFERENCE set */
  const cimq_lsq_desc* lsq;   /* wprep as for cimq_module_forward_codes */
  const float* weight;
  const float* alpha_act;
  const float* alpha_weight;
  const float* alpha_cim;
  const float* beta_cim;
  const int8_t* binary_mask;
  const float* signed_act;
  const float* scale; /* cimq_epilogue's scale, shift, flags */
  const float* shift;
  int32_t epi_flags;
  int32_t in_slot;    /* -1: the net's input x; else an activation slot */
  int32_t in_codes;   /* 1: read the slot's code plane (x_codes) */
  int32_t out_slot;
  int32_t out_mode;   /* 1 float, 2 codes, 3 both; the codes are for layer ``consumer``'s quantiser */
  int32_t consumer;   /* a layer index in (i, n_layers) whose in_slot is this out_slot; used when out_mode & 2 */
  int32_t res_slot;   /* -1: no residual; else the slot whose float plane is the residual's source */
  int32_t res_c0;     /* the output channel that the source's channel 0 adds to */
  int32_t res_stride; /* 1 or 2 */
  int32_t reserved;   /* 0 */
  void* ctx;          /* this layer's ctx (cimq_query_sizes), caller-owned */
} cimq_net_layer;

typedef struct cimq_net_head { /* global average pool over H x W, then y = W p + b */
  int32_t in_slot;     /* the slot whose float plane is pooled; -1: x itself (a head-only net, n_layers == 0) */
  int32_t classes;
  const float* weight; /* [classes, C] */
  const float* bias;   /* NULL or [classes] */
  float* pooled;       /* NULL, or [B, C]: the pooled features, also written */
  int32_t reserved[2]; /* 0 */
} cimq_net_head;

typedef struct cimq_net_desc {
  int32_t n_layers, n_slots;
  const cimq_net_layer* layers;
  const cimq_net_head* head; /* may be NULL */
  int32_t B, C, H, W;        /* shape of x */
} cimq_net_desc;

/* 1 where the cimq_net_* calls exist (a library from before them has no such symbol). */
int cimq_net_abi(void);

/* Validates the plan (as cimq_net_forward does, but for the buffers) and reports, per slot, the bytes of the largest
 * float plane and of the largest code plane stored in it (0 where that plane is never stored) -- two arrays of
 * n_slots entries, either may be NULL -- and the shared workspace: the largest of the layers' forward workspaces
 * (the head needs none). */
int cimq_net_sizes(const cimq_net_desc* net, size_t* slot_float_bytes, size_t* slot_code_bytes, size_t* ws_bytes);

/* Runs the plan on ``stream``: the layers in order, then the head into logits [B, classes].  slot_float /
 * slot_codes: host arrays of n_slots device pointers (an entry may be NULL where cimq_net_sizes reports 0; either
 * array may be NULL when n_slots is 0).  The plan is validated completely before the first launch and a refused plan
 * launches nothing.  The call allocates nothing, does not synchronise and reads no device memory on the host.
 * CIMQ_EINVAL: a NULL where a pointer is required; n_layers < 0, or n_layers == 0 without a head; a slot index out of
 * range; a layer or head reading a slot, or a plane of a slot, that no earlier layer wrote; a producer's output shape
 * that differs from the consumer's descriptor or from x's; out_slot equal to the layer's in_slot or res_slot; a
 * consumer outside (i, n_layers) or whose in_slot is not this out_slot; out_mode outside 1..3; in_codes outside 0..1;
 * res_stride not 1 or 2; a residual source whose [ceil(Hr / s), ceil(Wr / s)] is not [Ho, Wo] or whose batch is not
 * B; res_c0 < 0 or res_c0 + Cr > O; a non-zero reserved; a buffer that is not 16-byte aligned; classes < 1; every
 * refusal of the per-layer call.  CIMQ_EUNSUPPORTED: what cimq_module_codes_supported refuses; a stochastic-ADC layer
 * (its seed is per call); a residual view (res_stride 2, or Cr != O) on the dense route, or on the fwd5 / v3 routes
 * with an output width that is no multiple of 4; a head over more than CIMQ_NET_HEAD_MAX_C channels. */
int cimq_net_forward(const cimq_net_desc* net, const float* x, void* const* slot_float, void* const* slot_codes,
                     float* logits, void* ws, void* stream);

/* cimq_net_ext.head_flags */
#define CIMQ_NET_HEAD_FLATTEN 1 /* the head reads its slot's [B, C, H, W] plane as [B, C*H*W, 1, 1]: y = W flat(x) + b */

/* What a plan may add without moving cimq_net_layer / _head / _desc (cimq_pool_abi() == 1): pooled layers and a
 * classifier over the flattened map (VGG).  A layer with pool[i] == CIMQ_POOL_MAX2 is the cimq_module_forward_pool
 * call: its slot holds [B, O, Ho/2, Wo/2] -- the shape its consumers' descriptors, cimq_net_sizes_ex's bytes and the
 * head see -- while its residual, a whole tensor, has the unpooled shape. */
typedef struct cimq_net_ext {
  const int32_t* pool;   /* NULL, or n_layers entries: 0, or CIMQ_POOL_MAX2 for that layer's output */
  int32_t head_flags;    /* CIMQ_NET_HEAD_FLATTEN (1): the head reads its slot's [B,C,H,W] plane as [B, C*H*W, 1, 1] */
  int32_t reserved[3];   /* 0 */
} cimq_net_ext;

/* cimq_net_sizes / cimq_net_forward with ``ext``; ext == NULL is that call exactly.  On top of its refusals, all
 * before the first launch -- CIMQ_EINVAL: a pool entry other than 0 / CIMQ_POOL_MAX2, unknown head_flags, a non-zero
 * reserved.  CIMQ_EUNSUPPORTED: a pooled layer for which cimq_module_pool_supported answers 0 (a pooled layer with
 * out_mode & 2 or a residual view is the wide route's own refusal); a flatten head over more than
 * CIMQ_NET_HEAD_MAX_C features (C*H*W; with the flag, head->pooled is [B, C*H*W]).
 *
 * One more thing a non-NULL ext changes, an all-zero one included: which kernel a w8a8 layer on CIMQ_ROUTE_V3 runs
 * (eight 1-bit slices a side, the library ADC, a float-only edge, W % 4 == 0: the first conv of the CIFAR networks, in
 * a ResNet plan as in a VGG one).  Under cimq_net_forward and the per-layer calls such a layer is two launches: the
 * activation prologue, which writes the slice words of x into its ctx, then the forward.  In a cimq_net_forward_ex
 * plan the forward kernel quantises x in its own row staging (an instance of its own, the prologue's element chain)
 * and the prologue is not launched: one launch for a prepared layer, the same plane bit for bit, the same sizes; the
 * ctx's slice-word region goes unwritten.  cimq_module_forward_form's answer for the layer (form[1] == 0) describes
 * the per-layer calls and is unchanged.  VGG-small with q->wprep set on every layer is so 7 kernels: 6 convs + head. */
int cimq_net_sizes_ex(const cimq_net_desc* net, size_t* slot_float_bytes, size_t* slot_code_bytes, size_t* ws_bytes,
                      const cimq_net_ext* ext);
int cimq_net_forward_ex(const cimq_net_desc* net, const float* x, void* const* slot_float, void* const* slot_codes,
                        float* logits, void* ws, void* stream, const cimq_net_ext* ext);

/* One layer of cimq_module_prepare: its descriptors (as the forward will receive them; the
 * lsq descriptor's wprep and flags are ignored here) and raw parameters, and its output buffer
 * ``wprep`` (cimq_sizes.wprep_bytes, caller-owned device memory). */
typedef struct cimq_prepare_item {
  const cimq_conv_desc* desc;
  const cimq_lsq_desc* lsq;
  const float* weight;
  const float* alpha_act;
  const float* alpha_weight;
  const float* alpha_cim; /* NULL unless adc_bits is 1 or 1.5 */
  const int8_t* binary_mask;
  void* wprep;
} cimq_prepare_item;

/* The weight side of cimq_module_forward for n layers at once (lsq.py:552-571: w_q, alpha_q and
 * the step sizes, turned into the CiM kernels' operands and ADC / STE thresholds): one launch per
 * up to 7 layers instead of a few latency-bound workgroups inside every layer's prologue.  A
 * forward given q->wprep = items[i].wprep must see the same parameter values (e.g. prepare after
 * each optimizer step); the backward of that forward reads the buffer too, so it must not be
 * re-prepared in between. */
int cimq_module_prepare(int n, const cimq_prepare_item* items, void* stream);

/* One layer of cimq_module_prepare_shift: cimq_prepare_item's fields, and the shift ADC's beta_cim. */
typedef struct cimq_prepare_shift_item {
  const cimq_conv_desc* desc; /* CIMQ_OPT_INFERENCE set, adc_variant CIMQ_ADC_SHIFT_ROUND */
  const cimq_lsq_desc* lsq;
  const float* weight;
  const float* alpha_act;
  const float* alpha_weight;
  const float* alpha_cim; /* required */
  const int8_t* binary_mask;
  void* wprep;
  const float* beta_cim;  /* required, [1, T, nbw, nba, 1, O] */
  int32_t reserved[2];    /* 0 */
} cimq_prepare_shift_item;

/* 1 where cimq_module_prepare_shift exists and the forward-only shift calls take q->wprep (a library from before
 * them has no such symbol).  CIMQ_ABI_VERSION / _MINOR and cimq_net_abi() are unchanged. */
int cimq_shift_prepare_abi(void);

/* cimq_module_prepare for forward-only layers of the fused shift ADC (cimq_module_shift_supported): the same
 * packing and the same wprep_bytes, with beta_cim folded into the ADC thresholds, the per-channel beta sums and the
 * literal-ADC flag of a non-finite beta in the buffer.  cimq_module_shift_forward, cimq_module_forward_epilogue /
 * _codes with beta_cim and a shift layer of a cimq_net_forward plan, given q->wprep = items[i].wprep, skip their
 * weight blocks and write ``out`` / ``out_codes`` bit for bit as with q->wprep NULL; where the forward also
 * quantises the activation in its own staging the layer is then one launch.  CIMQ_EINVAL: a NULL beta_cim or
 * alpha_cim, a non-zero reserved, a descriptor without CIMQ_OPT_INFERENCE (the shift backward reads nothing
 * prepared), a NULL among the other pointers.  CIMQ_EUNSUPPORTED: a descriptor cimq_module_shift_supported answers
 * 0 for.  cimq_module_prepare itself refuses shift descriptors. */
int cimq_module_prepare_shift(int n, const cimq_prepare_shift_item* items, void* stream);

/* Opaque, caller-owned host memory for cimq_module_backward_chain: zero-initialise it once.
 * 16 KB since ABI 11. */
typedef struct cimq_pending {
  uint64_t opaque[2048];
} cimq_pending;

/* cimq_module_backward for a chain of layers run back to back on ONE stream (a network's
 * backward pass): the parameter-gradient epilogue of each call (the grad_w / grad_alpha slab
 * sums, the LSQ and alpha_cim quantiser backwards) is not launched but left in ``pending``;
 * cimq_pending_flush launches every pending epilogue at once, packed: ceil(n/20) slab-sum (tail)
 * launches, the jobs sorted by slab count, then ceil(n/24) finish launches (since ABI 11; before,
 * each ran inside the next call's kernels).  A call also issues the pending ones first when 32 are
 * pending or when a pending one writes one of its gradient buffers.  The parameter gradients of a
 * call are therefore complete only after the flush (or a later call that issued them) has been
 * issued on the stream; every buffer the call used (ctx, ws, weight, alpha_cim, the four gradient
 * buffers) must stay valid and unreused until then -- in particular ``ws`` must not be handed to
 * another chained call before that.  Memory: each pending layer keeps its workspace alive, and a
 * workspace holds the layer's grad_w slabs (one per image on the fused / first-conv paths: about
 * 37.7 MB for a 64-channel ResNet-20 layer at B = 256), so the chain's peak is up to 32 workspaces;
 * flush more often (e.g. per segment of layers, as bench.Trainer does at world > 1) to bound it.
 * Same arguments as cimq_module_backward; CIMQ_LSQ_SKIP_TAIL and CIMQ_LSQ_DEFER_GW are refused. */
int cimq_module_backward_chain(const cimq_conv_desc* d, const cimq_lsq_desc* q, const float* grad_out,
                               const float* x, const float* weight, const float* alpha_act,
                               const float* alpha_weight, const float* alpha_cim, const int8_t* binary_mask,
                               const float* signed_act, const void* ctx, float* grad_x, float* grad_weight,
                               float* grad_alpha_act, float* grad_alpha_weight, float* grad_alpha_cim, void* ws,
                               cimq_pending* pending, void* stream);
int cimq_pending_flush(cimq_pending* pending, void* stream);
/* The number of epilogues ``pending`` holds (not yet issued).  After a chained call it is 1 when
 * every earlier one has been issued: the caller may then release their buffers.  Since ABI 11. */
int cimq_pending_jobs(const cimq_pending* pending);

/* First-step alpha_cim initialisation (lsq.py:557-563 with get_analog_partial_sums_signed,
 * lsq.py:35-87): alpha_init[1,T,nbw,nba,1,O] = 2*mean_{b,p}|ps*sw*sa| / sqrt(Qp_adc), zeros
 * replaced by sw*sa.  Uses x, w_q, sa, sw like cimq_forward (ctx is scratch here). */
int cimq_alpha_init(const cimq_conv_desc* d, const float* x, const float* w_q, const float* sa,
                    const float* sw, const int8_t* binary_mask, const float* signed_act,
                    float* alpha_init, void* ctx, void* ws, void* stream);

/* Forward of the scale + shift CiM conv (adc_variant CIMQ_ADC_SHIFT_ROUND / _SIGN): the
 * test Functions get_analog_partial_sums_autograd_ver2 / get_adcless_cim_output of
 * test/test_backward_cimlayer_scale_shift.py (:336-431 / :113-215) when x, w_q are the integer
 * x_int / w_int with sa = sw = 1, and this build's Conv2dLSQCiM(adc_shift=True) otherwise
 * (u = fp16(ps) * sw * sa as lsq.py:195 before the shifted ADC).  alpha and beta are
 * [1, T, nbw, nba, 1, O] fp32; the rest as cimq_forward. */
int cimq_shift_forward(const cimq_conv_desc* d, const float* x, const float* w_q, const float* sa,
                       const float* sw, const float* alpha, const float* beta, const int8_t* binary_mask,
                       const float* signed_act, float* out, void* ctx, void* ws, void* stream);

/* Backward of cimq_shift_forward (scale_shift.py:437-546 / :240-334): grad_x, grad_w, and
 * grad_alpha / grad_beta [1, T, nbw, nba, 1, O]; grad_sa as cimq_backward (RAW_LSQ only). */
int cimq_shift_backward(const cimq_conv_desc* d, const float* grad_out, const float* x, const float* sa,
                        const float* sw, const float* alpha, const float* beta, const int8_t* binary_mask,
                        const float* signed_act, const void* ctx, float* grad_x, float* grad_w,
                        float* grad_alpha, float* grad_beta, float* grad_sa, void* ws, void* stream);

/* Diagnostic / parity hook: cimq_forward that also writes every integer partial sum
 * ps_out[B,T,nbw,nba,P,O] (int32; the reference keeps them as the fp16 ctx.ps_int of
 * lsq.py:169-192) and its ADC output adc_out (same shape, fp32, before the shift-and-add
 * mask: adc_out of lsq.py:197-230).  Used by the bit-exactness tests. */
int cimq_debug_partial_sums(const cimq_conv_desc* d, const float* x, const float* w_q, const float* sa,
                            const float* sw, const float* alpha_q, const int8_t* binary_mask,
                            const float* signed_act, float* out, int32_t* ps_out, float* adc_out,
                            void* ctx, void* stream);

/* Parity hook for the production forward: decodes the per-partial-sum state words that the
 * fast forward (cim_fwd_v3_kernel on the v7 path) left in ``ctx`` -- the ADC code
 * (lsq.py:321-332: -1 / 0 / +1) and the STE pass bit (lsq.py:310-313) of every (tile, w-slice,
 * a-slice) partial sum -- into code_out / pass_out [B, T, nbw, nba, P, O] (int8 / uint8).
 * ``ctx`` must come from cimq_forward / cimq_module_forward with the same descriptor;
 * CIMQ_EUNSUPPORTED for layers whose forward writes no state words. */
int cimq_debug_state_codes(const cimq_conv_desc* d, const void* ctx, int8_t* code_out, uint8_t* pass_out,
                           void* stream);

/* Parity hook for the module layers whose backward recomputes the partial sums (CIMQ_ROUTE_R6, whose forward
 * leaves no state words): the ADC codes and STE pass bits as cimq_debug_state_codes gives them, produced by the
 * recomputing backward's own code path (cim_bwd_r6_kernel in its debug form) from x, signed_act and the ctx of
 * cimq_module_forward.  ``st_scratch`` is caller-owned device memory of T * B * Ho * Wo * O * 4 bytes.
 * CIMQ_EUNSUPPORTED for other layers.  Since ABI 13. */
int cimq_debug_recompute_codes(const cimq_conv_desc* d, const float* x, const float* signed_act, const void* ctx,
                               void* st_scratch, int8_t* code_out, uint8_t* pass_out, void* stream);

/* ---- plain LSQ modules (lsq.py:389-436 Conv2dLSQ, :591-617 LinearLSQ, :620-662 ActLSQ) ---- */

/* The LSQ quantiser out = round_pass(clamp(x / s, qn, qp)) [* s if scaled] over n fp32
 * elements (any float-aligned x, out: 16-byte aligned ones take vector loads), s = *s the grad-scaled step size (grad_scale(alpha, g),
 * lsq.py:407-412 / :608-611 / :653-656, evaluated by the caller).  Replaces those lines'
 * torch ops: ActLSQ's codes (scaled = 0), Conv2dLSQ's weight codes (0), LinearLSQ's w_q (1). */
int cimq_lsq_quantize_forward(const float* x, long long n, const float* s, float qn, float qp, int scaled,
                              float* out, void* stream);

/* Autograd of cimq_lsq_quantize_forward: grad_x (STE through round_pass, the clamp mask,
 * DivBackward wrt x) and grad_s[1] = d loss / d s (MulBackward's sum when scaled, then
 * DivBackward's -grad_t * ((x / s) / s)), reduced in a fixed order.  ``ws`` holds
 * cimq_lsq_quantize_workspace_bytes(n). */
size_t cimq_lsq_quantize_workspace_bytes(long long n);
int cimq_lsq_quantize_backward(const float* x, long long n, const float* s, float qn, float qp, int scaled,
                               const float* grad_out, float* grad_x, float* grad_s, void* ws, void* stream);

/* Conv2dLSQ's conv of integer codes (lsq.py:436): x_codes [B,C,H,W] and w_codes [O,C,KH,KW]
 * are fp32 tensors holding integers (ActLSQ / weight-quantiser codes) in [code_min, code_max]
 * (activations) and [-128, 127] (weights). */
typedef struct cimq_qconv_desc {
  int32_t batch, in_channels, in_h, in_w;
  int32_t out_channels, kernel_h, kernel_w;
  int32_t stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, groups; /* groups must be 1 */
  int32_t code_min, code_max; /* activation code range: within [-128, 127] or [0, 255] */
  int32_t has_bias;
  int32_t reserved;
} cimq_qconv_desc;

int cimq_qconv_sizes(const cimq_qconv_desc* d, size_t* fwd_workspace_bytes, size_t* bwd_workspace_bytes);

/* y0 = conv2d(x_codes, w_codes) (+ bias) on int8 MFMA (exact int32 sums, then fp32; the
 * reference's fp32 conv of the same integers is exact while |sum| < 2^24) and
 * y = (y0 * act_scale) * w_scale, both [B, O, Ho, Wo].  y0 is kept for the backward (the
 * tensor torch's MulBackward saves).  act_scale / w_scale: device pointers to one float. */
int cimq_qconv_forward(const cimq_qconv_desc* d, const float* x_codes, const float* w_codes, const float* act_scale,
                       const float* w_scale, const float* bias, float* y, float* y0, void* ws, void* stream);

/* Elementwise backward of y = (y0 * act_scale) * w_scale: grad_y0 = (grad_y * w_scale) * act_scale,
 * grad_scales[0] = sum grad_y * (y0 * act_scale) (d / d w_scale), grad_scales[1] =
 * sum (grad_y * w_scale) * y0 (d / d act_scale).  The conv's own input / weight gradients of
 * grad_y0 are plain fp32 convolutions (the caller's library conv). */
int cimq_qconv_backward_scales(const cimq_qconv_desc* d, const float* grad_y, const float* y0, const float* act_scale,
                               const float* w_scale, float* grad_y0, float* grad_scales, void* ws, void* stream);

/* Diagnostic kernel timer.  Until cimq_profile_stop(), every launch of kernel ``kernel_id``
 * (1 = partial-sum forward, 2 = grad_x, 3 = grad_w/grad_alpha, 4 = act-code prep, each over
 * all kernel variants; 5 / 6 / 7 = only the v7-path forward / grad_x / grad_w kernels; 8 = the
 * fused backward of the stride-1 w2a2 / w3a3 layers, role 2) is
 * bracketed by a hipEvent pair on its launch stream (at most ``max_launches``).  stop()
 * waits for the last event and returns the summed kernel time, the number of launches and
 * their summed algorithmic bytes / flops ("Roofline accounting"). */
int cimq_profile_start(int kernel_id, int max_launches);
int cimq_profile_stop(double* total_ms, int* launches, double* algo_bytes, double* algo_flops);
/* ABI 9: before cimq_profile_stop(), the first ``cap`` launches one by one -- HIP-event duration (ms),
 * the SURVEY 8(d) algorithmic bytes and logical flops, and the MFMA operations as issued (int8 bit-slice
 * products of the live slice pairs forward, three bf16 products per fp32-accurate backward MAC) -- and
 * in *launches the count recorded.  Lets a caller take max(t_HBM, t_MFMA) per launch. */
int cimq_profile_read(int cap, double* ms, double* algo_bytes, double* algo_flops, double* mfma_ops, int* launches);

/* One SGD step (momentum, per-element weight decay, no dampening / Nesterov: torch.optim.SGD's
 * update, examples/__init__.py:184-188) over n flat fp32 elements in one launch:
 *   d = grad + wd * param;  buf = first ? d : momentum * buf + d;  param -= lr * buf
 * (each operation rounded to fp32, no fused multiply-adds), then grad = 0 when zero_grad is set.
 * The bench's optimizer (dist.FlatSGD) on the flat parameter / gradient buffers.  Since ABI 11. */
int cimq_flat_sgd(long long n, float* param, float* grad, float* buf, const float* wd, float lr, float momentum,
                  int first, int zero_grad, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CIMQ_H */
