// cimq_api.hip -- the extern "C" boundary of libcimq.so (declared in include/cimq.h).
// Host-side geometry validation, ctx / workspace carving and the kernel launch sequences
// that replace get_cim_output_signed.forward / backward (models/_modules/lsq.py:92-386).
#include <vector>

#include "cimq_host.h"
#include "cimq_prep.hip"
#include "cimq_lsq.hip"

using namespace cimq;

namespace {

// the entry points with no forward-only form refuse CIMQ_OPT_INFERENCE before they look at any other argument
int refuse_inference(const cimq_conv_desc* d, const char* who) {
  if (d && (d->options & CIMQ_OPT_INFERENCE))
    return fail(CIMQ_EINVAL, "%s: CIMQ_OPT_INFERENCE descriptors are forward only (cimq_forward, cimq_module_forward, "
                             "cimq_module_shift_forward, cimq_module_prepare)", who);
  return CIMQ_OK;
}

int prep_all(const Geo& g, const float* x, const float* w_q, const float* sa, const float* sw,
             const float* alpha_q, const int8_t* bmask, const float* signed_act, uint8_t* ctx,
             hipStream_t s, bool need_params, bool need_wgx, const float* beta = nullptr) {
  CtxLayout L = ctx_layout(g);
  const Route r = route_of(g);
  const int blk = 256;
  if (!r.actq) {  // (there the forward's row staging quantises, and the ctx has no slice words)
    // one 4-element item per thread up to 8192 blocks (fewer, fatter blocks measured slower)
    int grid = cdiv(g.Nin, 4 * blk);
    if (grid > act_blocks()) grid = act_blocks();
    const int slot = prof_begin(KID_PREP_ACT, g, s);
    if (g.inference)  // forward only: the forward slice words alone (the ctx has no backward words)
      hipLaunchKernelGGL(prep_act_fwd_kernel, dim3(grid), dim3(blk), 0, s, g, x, sa, signed_act, ctx + L.xcode);
    else
      hipLaunchKernelGGL(prep_act_kernel, dim3(grid), dim3(blk), 0, s, g, x, sa, signed_act,
                         ctx + L.xcode, ctx + L.xhat);
    prof_end(slot, s);
    CIMQ_TRY(check_hip("prep_act"));
  }
  {
    int total = g.T * g.KS * g.NBLK * 64;
    hipLaunchKernelGGL(prep_wfrag_kernel, dim3(cdiv(total, blk)), dim3(blk), 0, s, g, w_q, sw,
                       reinterpret_cast<v4i*>(wreg(g, ctx) + L.wfrag));
    CIMQ_TRY(check_hip("prep_wfrag"));
  }
  // the backward's weight operands (none in a forward-only call; need_wgx: the alpha_cim init has no backward)
  if (need_wgx && r.wgx) {
    int total = g.T * g.FBT * g.NKS * 64;
    hipLaunchKernelGGL(prep_wgx_kernel, dim3(cdiv(total, blk)), dim3(blk), 0, s, g, w_q, sw,
                       reinterpret_cast<v4i*>(wreg(g, ctx) + L.wgx));
    CIMQ_TRY(check_hip("prep_wgx"));
  }
  if (need_wgx && r.wcy) {
    const int ncpbt = v7_plan(g).v.NCPBT;
    const int tc = g.T * ncpbt * g.NKS * 64;
    hipLaunchKernelGGL(prep_wcy_kernel, dim3(cdiv(tc, blk)), dim3(blk), 0, s, g, w_q, sw, ncpbt,
                       reinterpret_cast<v4i*>(wreg(g, ctx) + L.wcy));
    CIMQ_TRY(check_hip("prep_wcy"));
  }
  // cim_bwd_gx5_kernel's operand (the RAW_LSQ Function path runs that kernel too)
  if (need_wgx && r.wg5) CIMQ_TRY(launch_prep_wg5(g, w_q, sw, ctx, s));
  Params pp = params_of(g, ctx);
  if (need_params) {
    if (hipMemsetAsync(pp.flags, 0, 16, s) != hipSuccess) return fail(CIMQ_EHIP, "memset flags");
    int total = g.T * g.nba * g.nbw * g.Opad + g.nbw * g.nba + (beta != nullptr ? g.Opad : 0);
    hipLaunchKernelGGL(prep_params_kernel, dim3(cdiv(total, blk)), dim3(blk), 0, s, g, alpha_q, sw, sa,
                       bmask, pp, beta);
    CIMQ_TRY(check_hip("prep_params"));
  }
  return CIMQ_OK;
}

// The backward kernels of the layer's route.  parts: bit 0 grad_x (with everything a single-pass backward
// produces), bit 1 grad_w where that is a launch of its own (Route::gw_own: with CIMQ_LSQ_DEFER_GW it leaves
// cimq_module_backward for cimq_module_backward_params)
int dispatch_bwd_any(const Geo& g, const uint8_t* ctx, const float* sw, const float* sa, const float* signed_act,
                     const float* gout, const float* x, float* gx, uint8_t* ws, hipStream_t s, int parts = 3) {
  const Route r = route_of(g);
  if (parts != 3 && !r.gw_own) return fail(CIMQ_EINVAL, "internal: grad_w alone on a single-pass backward");
  switch (r.gx) {
    case CIMQ_ROUTE_R6:  // the module path's w3a3 16-channel layers: recompute, no state words (cimq_r6.hip)
      if (!signed_act) return fail(CIMQ_EINVAL, "internal: the recompute backward needs signed_act");
      return launch_r6(g, r6_plan(g), ctx, sw, sa, signed_act, gout, x, gx, ws, s);
    case CIMQ_ROUTE_C1: return launch_c1(g, c1_plan(g), ctx, sw, sa, gout, x, gx, ws, s, r.lsq_fused);
    case CIMQ_ROUTE_FUSED: return launch_fused(g, v9_plan(g), ctx, sw, sa, gout, x, gx, ws, s, r.lsq_fused);
    case CIMQ_ROUTE_GX5:
    case CIMQ_ROUTE_V7:
      if (g.NBP == 8) return launch_v7_n<8, 8>(g, v7_plan(g), ctx, sw, sa, gout, x, gx, ws, s, parts);
      if (g.nbw == 2) return launch_v7_n<2, 2>(g, v7_plan(g), ctx, sw, sa, gout, x, gx, ws, s, parts);
      if (g.nbw == 4) return launch_v7_n<4, 4>(g, v7_plan(g), ctx, sw, sa, gout, x, gx, ws, s, parts);
      return launch_v7_n<3, 3>(g, v7_plan(g), ctx, sw, sa, gout, x, gx, ws, s, parts);
    case CIMQ_ROUTE_DENSE: return launch_dense_bwd(g, ctx, sw, gout, gx, ws, s, r.lsq_fused ? x : nullptr, sa);
    case CIMQ_ROUTE_GENERAL: return launch_bwd_general(g, ctx, sw, sa, signed_act, gout, x, gx, ws, s);
    default: return fail(CIMQ_EINVAL, "internal: a forward-only descriptor has no backward");
  }
}

// grad_w = sa * (slab sum over the backward's pixel chunks)
int launch_reduce_gw(const Geo& g, const float* sa, uint8_t* ws, float* grad_w, hipStream_t s) {
  WsLayout W = ws_layout(g);
  const long long nout = (long long)g.T * g.FBT * 16 * g.Opad;
  hipLaunchKernelGGL(reduce_gw_v3_kernel, dim3(cdiv(nout, 64)), dim3(1024), 0, s, g, W.nchunks_bwd,
                     reinterpret_cast<const float*>(ws + W.gw_slab), sa, grad_w);
  return check_hip("reduce_gw");
}

// the act-LSQ partials of the backward just run, Route::act_parts of them in the workspace: left by the grad_x
// kernel, or by the separate pass over grad_x here; grad_sa: their sum (nullptr: a module epilogue sums them)
int launch_act_lsq(const Geo& g, const float* x, const float* sa, float* grad_x, uint8_t* ws, float* grad_sa,
                   hipStream_t s) {
  const Route r = route_of(g);
  float* part = reinterpret_cast<float*>(ws + ws_layout(g).lsq_part);
  if (!r.lsq_fused) {
    hipLaunchKernelGGL(lsq_act_bwd_kernel, dim3(r.act_parts), dim3(256), 0, s, g.Nin, x, sa, g.lsq_qp, grad_x, part);
    CIMQ_TRY(check_hip("lsq_act_bwd"));
  }
  if (!grad_sa) return CIMQ_OK;
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, s, r.act_parts, part, grad_sa);
  return check_hip("sum_partials");
}

int launch_reduce_galpha(const Geo& g, const uint8_t* ctx, uint8_t* ws, float cgrad, int init, const float* sw,
                         const float* sa, float* out, hipStream_t s) {
  WsLayout W = ws_layout(g);
  const long long nout = (long long)g.T * g.nbw * g.nba * g.Opad;
  hipLaunchKernelGGL(reduce_galpha_v3_kernel, dim3(cdiv(nout, 64)), dim3(1024), 0, s, g, init ? W.nchunks : W.nchunks_bwd,
                     reinterpret_cast<const float*>(ws + W.ga_slab), params_of(g, const_cast<uint8_t*>(ctx)),
                     cgrad, init, sw, sa, (float)((double)g.B * g.P), (float)sqrt((double)g.qp), out);
  return check_hip("reduce_galpha");
}

// mask * cgrad * (slab sum over the backward's pixel chunks) -> [1, T, nbw, nba, 1, O]
int launch_reduce_slab(const Geo& g, const uint8_t* ctx, uint8_t* ws, size_t slab, float cgrad, const float* sw,
                       const float* sa, float* out, hipStream_t s) {
  WsLayout W = ws_layout(g);
  const long long nout = (long long)g.T * g.nbw * g.nba * g.Opad;
  hipLaunchKernelGGL(reduce_galpha_v3_kernel, dim3(cdiv(nout, 64)), dim3(1024), 0, s, g, W.nchunks_bwd,
                     reinterpret_cast<const float*>(ws + slab), params_of(g, const_cast<uint8_t*>(ctx)), cgrad, 0,
                     sw, sa, 1.f, 1.f, out);
  return check_hip("reduce_slab");
}

}  // namespace

extern "C" {

int cimq_abi_version(void) { return CIMQ_ABI_VERSION; }
int cimq_abi_minor(void) { return CIMQ_ABI_MINOR; }

const char* cimq_last_error(void) { return g_last_error.c_str(); }

int cimq_query_sizes(const cimq_conv_desc* d, cimq_sizes* out) {
  Geo g;
  CIMQ_TRY(make_geo(d, &g));
  if (!out) return fail(CIMQ_EINVAL, "null output");
  out->ctx_bytes = ctx_layout(g).total;
  out->wprep_bytes = ctx_layout(g).wbytes;
  WsLayout W = ws_layout(g);
  out->fwd_workspace_bytes = W.total;
  out->bwd_workspace_bytes = g.inference ? 0 : W.total;  // (forward only: there is no backward)
  // the module entry points' ctx: no state words where their backward recomputes them
  out->module_ctx_bytes = ctx_layout(module_form(g)).total;
  return CIMQ_OK;
}

int cimq_forward(const cimq_conv_desc* d, const float* x, const float* w_q, const float* sa,
                 const float* sw, const float* alpha_q, const int8_t* binary_mask,
                 const float* signed_act, float* out, void* ctx, void* ws, void* stream) {
  Geo g;
  CIMQ_TRY(make_geo(d, &g));
  if (!x || !w_q || !sa || !sw || !binary_mask || !signed_act || !out || !ctx)
    return fail(CIMQ_EINVAL, "null pointer argument");
  if ((g.mode == ADC_SIGN || g.mode == ADC_TERNARY) && !alpha_q)
    return fail(CIMQ_EINVAL, "adc_bits 1 / 1.5 need alpha_q");
  if (g.variant == VAR_SHIFT_ROUND || g.variant == VAR_SHIFT_SIGN)
    return fail(CIMQ_EINVAL, "scale/shift ADC variants go through cimq_shift_forward");
  (void)ws;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  uint8_t* c = reinterpret_cast<uint8_t*>(ctx);
  // forward only (CIMQ_OPT_INFERENCE): no backward weight operands; the activation quantiser in the forward's
  // row staging where that applies (Route::actq: the same words, bit for bit, without the pass over x)
  CIMQ_TRY(prep_all(g, x, w_q, sa, sw, alpha_q, binary_mask, signed_act, c, s, true, true));
  const ActQ aq{x, signed_act};
  return launch_fwd_any(g, c, sw, sa, out, nullptr, nullptr, s, route_of(g).actq ? &aq : nullptr);
}

int cimq_shift_forward(const cimq_conv_desc* d, const float* x, const float* w_q, const float* sa,
                       const float* sw, const float* alpha, const float* beta, const int8_t* binary_mask,
                       const float* signed_act, float* out, void* ctx, void* ws, void* stream) {
  CIMQ_TRY(refuse_inference(d, "cimq_shift_forward"));
  Geo g;
  CIMQ_TRY(make_geo(d, &g));
  if (g.variant != VAR_SHIFT_ROUND && g.variant != VAR_SHIFT_SIGN)
    return fail(CIMQ_EINVAL, "cimq_shift_forward needs adc_variant CIMQ_ADC_SHIFT_ROUND or _SIGN");
  if (!x || !w_q || !sa || !sw || !alpha || !beta || !binary_mask || !signed_act || !out || !ctx)
    return fail(CIMQ_EINVAL, "null pointer argument");
  (void)ws;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  uint8_t* c = reinterpret_cast<uint8_t*>(ctx);
  CIMQ_TRY(prep_all(g, x, w_q, sa, sw, alpha, binary_mask, signed_act, c, s, true, true, beta));
  return launch_fwd_any(g, c, sw, sa, out, nullptr, nullptr, s);
}

int cimq_shift_backward(const cimq_conv_desc* d, const float* grad_out, const float* x, const float* sa,
                        const float* sw, const float* alpha, const float* beta, const int8_t* binary_mask,
                        const float* signed_act, const void* ctx, float* grad_x, float* grad_w,
                        float* grad_alpha, float* grad_beta, float* grad_sa, void* ws, void* stream) {
  CIMQ_TRY(refuse_inference(d, "cimq_shift_backward"));
  Geo g;
  CIMQ_TRY(make_geo(d, &g));
  (void)alpha; (void)beta;
  if (g.variant != VAR_SHIFT_ROUND && g.variant != VAR_SHIFT_SIGN)
    return fail(CIMQ_EINVAL, "cimq_shift_backward needs adc_variant CIMQ_ADC_SHIFT_ROUND or _SIGN");
  if (!grad_out || !sa || !sw || !signed_act || !ctx || !grad_x || !grad_w || !grad_alpha || !grad_beta || !ws)
    return fail(CIMQ_EINVAL, "null pointer argument");
  if (g.input_kind == CIMQ_INPUT_RAW_LSQ && (!x || !grad_sa))
    return fail(CIMQ_EINVAL, "RAW_LSQ backward needs x and grad_sa");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint8_t* c = reinterpret_cast<const uint8_t*>(ctx);
  uint8_t* w = reinterpret_cast<uint8_t*>(ws);
  const Route r = route_of(g);
  if (r.shift_stats && !binary_mask) return fail(CIMQ_EINVAL, "null binary_mask");
  CIMQ_TRY(dispatch_bwd_any(g, c, sw, sa, signed_act, grad_out, x, grad_x, w, s));
  CIMQ_TRY(launch_reduce_gw(g, sa, w, grad_w, s));
  if (r.shift_stats) {
    // the shift ADC on the fast path (shift_fast): grad_x / grad_w from the state words as for the
    // library ADC (same STE mask), the step-size gradients from the statistics kernel
    CIMQ_TRY(launch_shift_stats(g, c, sw, sa, grad_out, binary_mask, w, grad_alpha, grad_beta, s));
  } else {
    // the general kernels.  grad_alpha: sign variant sum sign * G / sqrt(numel * Qp) (scale_shift.py:283); round
    // variant without the factor (:491 commented out); grad_beta: sum over the clamped region / all of G
    WsLayout W = ws_layout(g);
    const double numel = (double)g.B * g.T * g.nbw * g.nba * g.P * g.O;
    const float cgrad = g.variant == VAR_SHIFT_SIGN ? (float)(1.0 / sqrt(numel * (double)g.qp)) : 1.f;
    CIMQ_TRY(launch_reduce_slab(g, c, w, W.ga_slab, cgrad, sw, sa, grad_alpha, s));
    CIMQ_TRY(launch_reduce_slab(g, c, w, W.gb_slab, 1.f, sw, sa, grad_beta, s));
  }
  if (g.input_kind == CIMQ_INPUT_RAW_LSQ) CIMQ_TRY(launch_act_lsq(g, x, sa, grad_x, w, grad_sa, s));
  return CIMQ_OK;
}

int cimq_debug_partial_sums(const cimq_conv_desc* d, const float* x, const float* w_q, const float* sa,
                            const float* sw, const float* alpha_q, const int8_t* binary_mask,
                            const float* signed_act, float* out, int32_t* ps_out, float* adc_out, void* ctx,
                            void* stream) {
  CIMQ_TRY(refuse_inference(d, "cimq_debug_partial_sums"));
  Geo g;
  CIMQ_TRY(make_geo(d, &g));
  if (!x || !w_q || !sa || !sw || !binary_mask || !signed_act || !out || !ps_out || !adc_out || !ctx)
    return fail(CIMQ_EINVAL, "null pointer argument");
  if ((g.mode == ADC_SIGN || g.mode == ADC_TERNARY) && !alpha_q)
    return fail(CIMQ_EINVAL, "adc_bits 1 / 1.5 need alpha_q");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  uint8_t* c = reinterpret_cast<uint8_t*>(ctx);
  CIMQ_TRY(prep_all(g, x, w_q, sa, sw, alpha_q, binary_mask, signed_act, c, s, true, true));
  return launch_fwd_any(g, c, sw, sa, out, ps_out, adc_out, s);
}

int cimq_debug_state_codes(const cimq_conv_desc* d, const void* ctx, int8_t* code_out, uint8_t* pass_out,
                           void* stream) {
  CIMQ_TRY(refuse_inference(d, "cimq_debug_state_codes"));
  Geo g;
  CIMQ_TRY(make_geo(d, &g));
  if (!ctx || !code_out || !pass_out) return fail(CIMQ_EINVAL, "null pointer argument");
  const StateFmt fmt = route_of(g).state;
  if (fmt != ST_V7 && fmt != ST_V7X2 && fmt != ST_PLANES)
    return fail(CIMQ_EUNSUPPORTED,
                "this layer's forward writes no v7 state words: the hook decodes the 4-byte words of w2a2 / w3a3, "
                "the 8-byte words of w4a4 and the w8a8 planes (the first conv's backward recomputes them)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint8_t* c = reinterpret_cast<const uint8_t*>(ctx);
  const long long n = (long long)g.T * g.M * g.O;
  hipLaunchKernelGGL(decode_state_kernel, dim3(std::min(cdiv(n, 256), 8192)), dim3(256), 0, s, g,
                     fmt == ST_PLANES ? 1 : fmt == ST_V7X2 ? 2 : 0, c + ctx_layout(g).st, code_out, pass_out);
  return check_hip("decode_state");
}

int cimq_debug_recompute_codes(const cimq_conv_desc* d, const float* x, const float* signed_act, const void* ctx,
                               void* st_scratch, int8_t* code_out, uint8_t* pass_out, void* stream) {
  CIMQ_TRY(refuse_inference(d, "cimq_debug_recompute_codes"));
  Geo g;
  CIMQ_TRY(make_geo(d, &g));
  if (!x || !signed_act || !ctx || !st_scratch || !code_out || !pass_out) return fail(CIMQ_EINVAL, "null pointer argument");
  g.onchw = 1;  // the module entry points' layer
  if (route_of(g).gx != CIMQ_ROUTE_R6)
    return fail(CIMQ_EUNSUPPORTED, "this layer's module backward does not recompute the partial sums");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint8_t* c = reinterpret_cast<const uint8_t*>(ctx);
  const float* scal = reinterpret_cast<const float*>(wreg(g, c) + ctx_layout(g).lsq_scal);
  uint32_t* st = reinterpret_cast<uint32_t*>(st_scratch);
  CIMQ_TRY(launch_r6(g, r6_plan(g), c, scal + 1, scal, signed_act, nullptr, x, nullptr, nullptr, s, st));
  const long long n = (long long)g.T * g.M * g.O;
  hipLaunchKernelGGL(decode_state_kernel, dim3(std::min(cdiv(n, 256), 8192)), dim3(256), 0, s, g, 0,
                     reinterpret_cast<const uint8_t*>(st), code_out, pass_out);
  return check_hip("decode_state");
}

int cimq_backward(const cimq_conv_desc* d, const float* grad_out, const float* x, const float* sa,
                  const float* sw, const float* alpha_q, const int8_t* binary_mask,
                  const float* signed_act, const void* ctx, float* grad_x, float* grad_w,
                  float* grad_alpha, float* grad_sa, void* ws, void* stream) {
  CIMQ_TRY(refuse_inference(d, "cimq_backward"));
  Geo g;
  CIMQ_TRY(make_geo(d, &g));
  (void)alpha_q; (void)binary_mask;
  if (!grad_out || !sa || !sw || !signed_act || !ctx || !grad_x || !grad_w || !ws)
    return fail(CIMQ_EINVAL, "null pointer argument");
  if (g.variant == VAR_SHIFT_ROUND || g.variant == VAR_SHIFT_SIGN)
    return fail(CIMQ_EINVAL, "scale/shift ADC variants go through cimq_shift_backward");
  if (g.input_kind == CIMQ_INPUT_RAW_LSQ && (!x || !grad_sa))
    return fail(CIMQ_EINVAL, "RAW_LSQ backward needs x and grad_sa");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint8_t* c = reinterpret_cast<const uint8_t*>(ctx);
  uint8_t* w = reinterpret_cast<uint8_t*>(ws);
  CIMQ_TRY(dispatch_bwd_any(g, c, sw, sa, signed_act, grad_out, x, grad_x, w, s));
  CIMQ_TRY(launch_reduce_gw(g, sa, w, grad_w, s));
  if ((g.mode == ADC_SIGN || g.mode == ADC_TERNARY) && grad_alpha) {
    const double numel = (double)g.B * g.T * g.nbw * g.nba * g.P * g.O;
    const float cgrad = (float)(1.0 / sqrt(numel * (double)g.qp));  // lsq.py:323,330
    CIMQ_TRY(launch_reduce_galpha(g, c, w, cgrad, 0, sw, sa, grad_alpha, s));
  }
  if (g.input_kind == CIMQ_INPUT_RAW_LSQ) CIMQ_TRY(launch_act_lsq(g, x, sa, grad_x, w, grad_sa, s));
  return CIMQ_OK;
}

// the module backward's epilogue: grad_w + weight-LSQ backward, grad_alpha_cim, the step sizes;
// tail_blocks is the grid of its slab-sum launch
struct TailLaunch {
  int tail_blocks;
  Geo g;
  LsqArgs q;
  ModuleTail a;
};

static TailLaunch tail_job(const Geo& g, const LsqArgs& la, const cimq_lsq_desc* q, const uint8_t* c, uint8_t* w,
                      const float* weight, const float* alpha_cim, float* grad_weight, float* grad_alpha_act,
                      float* grad_alpha_weight, float* grad_alpha_cim, int gaq_ready = 0, bool packed = false) {
  const bool has_alpha = la.nbits_alpha > 0;
  CtxLayout L = ctx_layout(g);
  WsLayout W = ws_layout(g);
  TailLaunch j;
  memset(&j, 0, sizeof(j));
  ModuleTail& a = j.a;
  a.gw_slab = reinterpret_cast<const float*>(w + W.gw_slab);
  a.ga_slab = reinterpret_cast<const float*>(w + W.ga_slab);
  a.scal = reinterpret_cast<const float*>(wreg(g, c) + L.lsq_scal);
  a.weight = weight;
  a.alpha_cim = alpha_cim;
  a.apart = reinterpret_cast<float*>(w + W.lsq_part);
  a.wpart = reinterpret_cast<float*>(w + W.wpart);
  a.gaq = reinterpret_cast<float*>(w + W.gaq);
  a.grad_weight = grad_weight;
  a.grad_alpha_act = grad_alpha_act;
  a.grad_alpha_w = grad_alpha_weight;
  a.grad_alpha_cim = grad_alpha_cim;
  a.ckj = params_of(g, const_cast<uint8_t*>(c)).ckj;
  a.cgrad = (float)(1.0 / sqrt((double)g.B * g.T * g.nbw * g.nba * g.P * g.O * (double)g.qp));  // lsq.py:323,330
  a.nchunks = W.nchunks_bwd;
  // few chunks and many outputs (the dense path's 8 chunks of a 1024 x 1024 layer): one output per
  // thread (16 k blocks of 64 outputs each took 67 us for 34 MB of slab)
  const long long nout_w = (long long)g.T * g.FBT * 16 * g.Opad;
  a.wide = (a.nchunks <= 16 && nout_w >= (1 << 18) && tune("WIDE_SLAB", 1)) ? 1 : 0;
  // otherwise, in a launch packed with the other layers' epilogues (cimq_pending_flush), float4
  // reads in 64-lane rows, 256 outputs per block (reduce_chunks4; 16-lane rows there: 85.7 -> 92.6
  // us); alone, one output per lane, 64 per block, so that a small layer still spreads over the chip
  // (a layer's tail 6.8 us against 9.1 with the float4 rows, cfg4)
  a.lpr = packed ? tune("TAIL_LPR_PACKED", 64) : tune("TAIL_LPR_SINGLE", 0);
  const int per_blk = a.wide ? 1024 : a.lpr == 0 ? 64 : 4 * a.lpr;
  a.nwb = cdiv(nout_w, per_blk);
  a.nga = has_alpha ? cdiv((long long)g.T * g.nbw * g.nba * g.Opad, per_blk) : 0;
  a.napart = route_of(g).act_parts;
  a.accum = (q->flags & CIMQ_LSQ_ACCUMULATE_GRADS) ? 1 : 0;
  a.gapart = (has_alpha && la.nalpha > kFinishInReg && tune("WIDE_TAIL", 1)) ? reinterpret_cast<float*>(w + W.gapart) : nullptr;
  a.gaq_ready = gaq_ready;
  j.g = g;
  j.q = la;
  j.tail_blocks = a.nwb + a.nga;
  return j;
}

static int launch_tail(const TailLaunch& j, hipStream_t s) {
  hipLaunchKernelGGL(module_bwd_tail_kernel, dim3(j.tail_blocks), dim3(1024), 0, s, j.g, j.q, j.a);
  return check_hip("module_bwd_tail");
}

static int launch_finish(const TailLaunch& j, hipStream_t s) {
  if (j.a.gapart)
    hipLaunchKernelGGL(module_bwd_finish_wide_kernel, dim3(cdiv(j.q.nalpha, 1024)), dim3(1024), 0, s, j.q, j.a);
  else
    hipLaunchKernelGGL(module_bwd_finish_kernel, dim3(1), dim3(1024), 0, s, j.q, j.a);
  return check_hip("module_bwd_finish");
}

static int module_tail(Geo g, const LsqArgs& la, const cimq_lsq_desc* q, const uint8_t* c, uint8_t* w,
                       const float* weight, const float* alpha_cim, float* grad_weight, float* grad_alpha_act,
                       float* grad_alpha_weight, float* grad_alpha_cim, hipStream_t s, int gaq_ready = 0) {
  const TailLaunch j = tail_job(g, la, q, c, w, weight, alpha_cim, grad_weight, grad_alpha_act, grad_alpha_weight,
                           grad_alpha_cim, gaq_ready);
  CIMQ_TRY(launch_tail(j, s));
  return launch_finish(j, s);
}

// cimq_pending (caller-owned host memory): the epilogues chained module backwards left behind,
// in call order, with each one's tail grid
constexpr int kPendingJobs = 32;
struct Pending {
  uint32_t magic;
  int n;
  int nblk[kPendingJobs];
  TailJob job[kPendingJobs];
};
static_assert(sizeof(Pending) <= sizeof(cimq_pending), "cimq_pending too small");
constexpr uint32_t kPendingMagic = 0x63696d70u;

static TailJob tail_job_of(const TailLaunch& c) {
  TailJob t;
  t.t = TailGeo{c.g.T, c.g.FBT, c.g.Opad, c.g.O, c.g.xbar, c.g.K, c.g.nbw, c.g.nba};
  t.q = c.q;
  t.a = c.a;
  return t;
}

// every pending tail (packs of kTailJobs per launch), then every finish: the launch boundary
// orders each finish after its tail's partials
static int pending_run(Pending* pd, hipStream_t s) {
  if (pd->magic != kPendingMagic) return CIMQ_OK;
  const int n = pd->n;
  pd->magic = 0;
  pd->n = 0;
  // the jobs with the longest blocks (most chunks per output) first, so that the grid does not
  // end on a round of them; the jobs are independent (pending_overlaps), their order is free
  int ord[kPendingJobs];
  for (int i = 0; i < n; ++i) ord[i] = i;
  if (tune("TAIL_SORT", 1))
    std::stable_sort(ord, ord + n, [&](int x, int y) { return pd->job[x].a.nchunks > pd->job[y].a.nchunks; });
  for (int i = 0; i < n;) {
    TailPack tp;
    tp.n = 0;
    int blk = 0;
    for (; i < n && tp.n < kTailJobs; ++i, ++tp.n) {
      tp.blk0[tp.n] = blk;
      tp.job[tp.n] = pd->job[ord[i]];
      blk += pd->nblk[ord[i]];
    }
    tp.blk0[tp.n] = blk;
    hipLaunchKernelGGL(module_tail_many_kernel, dim3(blk), dim3(1024), 0, s, tp);
    CIMQ_TRY(check_hip("module_tail_many"));
  }
  for (int i = 0; i < n;) {
    FinishPack fp;
    fp.n = 0;
    int blk = 0;
    for (; i < n && fp.n < kFinishJobs; ++i, ++fp.n) {
      const TailJob& t = pd->job[i];
      fp.blk0[fp.n] = blk;
      fp.job[fp.n].q = t.q;
      fp.job[fp.n].a = t.a;
      blk += t.a.gapart ? cdiv(t.q.nalpha, 1024) : 1;
    }
    fp.blk0[fp.n] = blk;
    hipLaunchKernelGGL(module_finish_many_kernel, dim3(blk), dim3(1024), 0, s, fp);
    CIMQ_TRY(check_hip("module_finish_many"));
  }
  return CIMQ_OK;
}

// a pending epilogue writing any gradient buffer this one writes (a layer run twice in one
// backward): the two must not share a launch
static bool pending_overlaps(const Pending* pd, const ModuleTail& a) {
  for (int i = 0; i < pd->n; ++i) {
    const ModuleTail& b = pd->job[i].a;
    if (b.grad_weight == a.grad_weight || b.grad_alpha_act == a.grad_alpha_act || b.grad_alpha_w == a.grad_alpha_w ||
        (a.grad_alpha_cim && b.grad_alpha_cim == a.grad_alpha_cim))
      return true;
  }
  return false;
}

static int lsq_args(const Geo& g, const cimq_lsq_desc* q, LsqArgs* a) {
  if (!q) return fail(CIMQ_EINVAL, "null LSQ descriptor");
  if (!(q->qn_w < q->qp_w) || !(q->gscale_a > 0.f) || !(q->gscale_w > 0.f))
    return fail(CIMQ_EINVAL, "bad LSQ descriptor");
  if (q->nbits_alpha < 0 || q->nbits_alpha > 16 || q->nbits_alpha == 1)
    return fail(CIMQ_EINVAL, "nbits_alpha must be 0 (no alpha_cim) or 2..16");
  a->qn_w = q->qn_w;
  a->qp_w = q->qp_w;
  a->gs_a = q->gscale_a;
  a->gs_w = q->gscale_w;
  a->nbits_alpha = q->nbits_alpha;
  a->nalpha = g.T * g.nbw * g.nba * g.O;
  if (q->flags & ~(CIMQ_LSQ_ACCUMULATE_GRADS | CIMQ_LSQ_SKIP_TAIL | CIMQ_LSQ_DEFER_GW))
    return fail(CIMQ_EINVAL, "unknown LSQ flags 0x%x", q->flags);
  return CIMQ_OK;
}

// the module prologue's weight-side blocks: 256 items of its operands and parameter tables each, 1024 at the most
static int prep_wblocks(const ModulePrep& a) {
  return std::max(1, std::min(cdiv(a.nwf + a.nwg + a.nwc + a.nw5 + a.nwx5 + a.nwx6 + a.npp, 256), 1024));
}

// the module prologue's arguments: activation side into ctx c, weight side into wreg(g, c)
static ModulePrep module_prep_args(const Geo& g, const float* x, const float* weight, const float* alpha_act,
                                   const float* alpha_weight, const float* alpha_cim, const int8_t* binary_mask,
                                   const float* signed_act, uint8_t* c, int* nwblk) {
  CtxLayout L = ctx_layout(g);
  uint8_t* wr = wreg(g, c);
  const Route r = route_of(g);
  const Plan7 p7 = v7_plan(g);
  ModulePrep a;
  memset(&a, 0, sizeof(a));
  a.x = x;
  a.alpha_act = alpha_act;
  a.alpha_w = alpha_weight;
  a.weight = weight;
  a.alpha_cim = alpha_cim;
  a.signed_act = signed_act;
  a.bmask = binary_mask;
  a.xcf = c ? c + L.xcode : nullptr;
  a.xcb = (c && !g.inference) ? c + L.xhat : nullptr;  // (forward only: no backward words)
  a.wfrag = reinterpret_cast<v4i*>(wr + L.wfrag);
  a.wgx = reinterpret_cast<v4i*>(wr + L.wgx);
  a.wcy = reinterpret_cast<v4i*>(wr + L.wcy);
  a.pp = params_of(g, c);
  a.scal = reinterpret_cast<float*>(wr + L.lsq_scal);
  a.nact_blocks = (int)std::min<long long>(cdiv(g.Nin, 4 * 256), act_blocks());
  a.nwf = g.T * g.KS * g.NBLK * 64;
  // the backward's operands as the Route asks for them (none in a forward-only call)
  a.nwg = r.wgx ? g.T * g.FBT * g.NKS * 64 : 0;       // general / dense grad_x operand
  a.ncpbt = p7.ok ? p7.v.NCPBT : 1;
  a.nwc = r.wcy ? g.T * p7.v.NCPBT * g.NKS * 64 : 0;  // v8 grad_x operand
  const Plan5 p5 = f5_plan(g);
  a.wf5 = reinterpret_cast<v4i*>(wr + L.wf5);
  a.f5 = f5w_of(p5.v);
  a.nw5 = (int)f5_frag_items(g, p5);  // cim_fwd5_kernel's weight operand
  a.wg5 = reinterpret_cast<v4i*>(wr + L.wg5);
  a.nwx5 = r.wg5 ? (int)(x5_frag_bytes(g) / 16) : 0;  // cim_bwd_gx5_kernel's weight operand
  a.wx6 = reinterpret_cast<v4i*>(wr + L.wx6);
  a.nwx6 = r.wx6 ? (int)(r6_frag_bytes(g) / 16) : 0;  // cim_bwd_r6_kernel's gx operand
  a.npp = g.T * g.nba * g.nbw * g.Opad + g.nbw * g.nba;
  *nwblk = prep_wblocks(a);
  return a;
}

// the checks every module entry point shares, and the module form of the geometry (the output layout flag is
// fixed here: every entry point plans with the same Geo from its first line); applies q->wprep.  shift: the
// cimq_module_shift_* entry points (the shift ADC on the fast path; a prepared weight side -- cimq_module_prepare_shift
// -- in a forward-only call alone: the shift backward reads nothing prepared)
static int module_geo(const cimq_conv_desc* d, const cimq_lsq_desc* q, Geo* g, LsqArgs* la, bool shift = false) {
  CIMQ_TRY(make_geo(d, g));
  if (g->input_kind != CIMQ_INPUT_RAW_LSQ) return fail(CIMQ_EINVAL, "module entry points take the raw activation");
  *g = module_form(*g);
  if (shift) {
    if (g->variant != VAR_SHIFT_ROUND || !route_of(*g).shift_stats)
      return fail(CIMQ_EUNSUPPORTED, "cimq_module_shift_*: the shift ADC on a fast-path layer only "
                                     "(adc_variant CIMQ_ADC_SHIFT_ROUND, adc 1.5, 2 or 3 equal slices, v7 shapes)");
    if (q && q->wprep && !g->inference)
      return fail(CIMQ_EINVAL, "cimq_module_shift_*: no prepared weight side without CIMQ_OPT_INFERENCE");
  } else if (g->variant == VAR_SHIFT_ROUND || g->variant == VAR_SHIFT_SIGN) {
    return fail(CIMQ_EUNSUPPORTED, "the module entry points run the library / stochastic ADC only");
  }
  CIMQ_TRY(lsq_args(*g, q, la));
  g->wbase = reinterpret_cast<const unsigned char*>(q->wprep);
  return CIMQ_OK;
}

// alpha_cim is the sign / ternary ADC's scale (adc 1 / 1.5): required there, with its gradient in a backward, and
// ignored elsewhere (la->nbits_alpha = 0 then says there is none)
static int check_alpha(const Geo& g, LsqArgs* la, const float* alpha_cim, const float* grad_alpha_cim, bool bwd = true) {
  if (g.mode != ADC_SIGN && g.mode != ADC_TERNARY) {
    la->nbits_alpha = 0;
    return CIMQ_OK;
  }
  if (!alpha_cim || (bwd && !grad_alpha_cim) || la->nbits_alpha == 0)
    return fail(CIMQ_EINVAL, bwd ? "adc 1 / 1.5 need alpha_cim and grad_alpha_cim" : "adc 1 / 1.5 need alpha_cim");
  return CIMQ_OK;
}

// The host refusals of an output epilogue that need no geometry, shared by cimq_module_forward_epilogue and
// cimq_module_forward_codes (who: the entry point's name in the message)
static const char who_epi[] = "cimq_module_forward_epilogue";
static int check_forward_only(const char* who, const cimq_conv_desc* d) {
  if (d && !(d->options & CIMQ_OPT_INFERENCE))
    return fail(CIMQ_EINVAL, "%s: a CIMQ_OPT_INFERENCE descriptor only (forward only)", who);
  return CIMQ_OK;
}
static int check_epilogue(const char* who, const cimq_epilogue* epi, const float* alpha_cim, const float* beta_cim) {
  if (!epi || !epi->scale || !epi->shift) return fail(CIMQ_EINVAL, "%s: null epilogue, scale or shift", who);
  if (epi->flags & ~CIMQ_EPI_RELU) return fail(CIMQ_EINVAL, "%s: unknown flags 0x%x", who, epi->flags);
  if (epi->reserved != 0) return fail(CIMQ_EINVAL, "%s: reserved must be 0", who);
  if (reinterpret_cast<uintptr_t>(epi->residual) % 16 != 0)
    return fail(CIMQ_EINVAL, "%s: residual must be 16-byte aligned", who);
  if (beta_cim && !alpha_cim) return fail(CIMQ_EINVAL, "%s: beta_cim needs alpha_cim", who);
  return CIMQ_OK;
}

// the kernels' form of a checked epilogue (codes and view fields zero)
static Epi epi_of(const cimq_epilogue* epi) {
  return Epi{epi->scale, epi->shift, epi->residual, (epi->flags & CIMQ_EPI_RELU) ? 1 : 0};
}

// a clamp maximum that codes can carry: an integer in [1, 254], so that the NaN code Qp + 1 fits a byte
static bool codes_qp_ok(float qp) { return qp >= 1.f && qp <= 254.f && qp == (float)(int)qp; }

static int module_forward_impl(const cimq_conv_desc* d, const cimq_lsq_desc* q, const float* x, const float* weight,
                               const float* alpha_act, const float* alpha_weight, const float* alpha_cim,
                               const float* beta_cim, const int8_t* binary_mask, const float* signed_act, float* out,
                               void* ctx, void* ws, void* stream, const Epi* ep = nullptr, bool dry = false,
                               int pool = 0, bool stage8 = false) {
  // dry (cimq_net_forward's validation pass): every refusal below, no launch
  // stage8 (a layer of a cimq_net_forward_ex plan): a w8a8 layer that can (fwd8_stage_ok) quantises x in its kernel's
  // row staging -- the prologue's words, one launch fewer; a hint, ignored where it does not apply
  // pool (cimq_module_forward_pool, a pooled layer of cimq_net_forward_ex; CIMQ_POOL_MAX2 or 0, with ep): out is the
  // 2x2 / stride-2 max pool of the epilogue's values, [B, O, Ho/2, Wo/2]
  Geo g;
  LsqArgs la;
  CIMQ_TRY(module_geo(d, q, &g, &la, beta_cim != nullptr));
  if (pool && (pool != CIMQ_POOL_MAX2 || !ep)) return fail(CIMQ_EINVAL, "internal: a pooled forward off its entry point");
  // the residual's extent: out's geometry, or the view's own (Epi::rview, cimq_net_forward alone)
  const ResView rv = ep ? res_view(ep->rvw0, ep->rvw1) : ResView{};
  const uintptr_t res_bytes = !ep ? 0 : ep->rvw1 ? (uintptr_t)g.B * rv.cr * rv.h * rv.w * 4 : (uintptr_t)g.M * g.O * 4;
  if (ep) {  // cimq_module_forward_epilogue: the residual has out's geometry
    if (!g.inference) return fail(CIMQ_EINVAL, "cimq_module_forward_epilogue: a CIMQ_OPT_INFERENCE descriptor only");
    if (ep->res && out) {
      const uintptr_t r0 = reinterpret_cast<uintptr_t>(ep->res), o0 = reinterpret_cast<uintptr_t>(out);
      const uintptr_t nb = (uintptr_t)g.M * g.O * (pool ? 1 : 4);  // (pooled: a quarter of the residual's extent)
      if (r0 < o0 + nb && o0 < r0 + res_bytes)
        return fail(CIMQ_EINVAL, "cimq_module_forward_epilogue: residual overlaps out");
    }
    if (ep->rvw1) {  // the view lives in the code instances of the fwd5, v3 and general routes
      const int fwd = route_of(g).fwd;
      if (fwd == CIMQ_ROUTE_WIDE)
        return fail(CIMQ_EUNSUPPORTED, "cimq_net_forward: the wide route reads no residual view");
      if (fwd == CIMQ_ROUTE_DENSE)
        return fail(CIMQ_EUNSUPPORTED, "cimq_net_forward: the dense route reads no residual view (res_stride 2 or "
                                       "fewer source channels than out_channels)");
      if (fwd != CIMQ_ROUTE_GENERAL && g.Wo % 4 != 0)
        return fail(CIMQ_EUNSUPPORTED, "cimq_net_forward: a residual view on the fwd5 / v3 routes needs an output "
                                       "width that is a multiple of 4 (it is %d)", g.Wo);
    }
  }
  const uint8_t* xq = ep ? ep->xq : nullptr;  // cimq_module_forward_codes: the input as codes, x ignored
  uint8_t* oq = ep ? ep->oq : nullptr;        // ... the output's codes; with nofloat, out is not written
  if (xq || oq) {
    const Route rc = route_of(g);
    if (rc.fwd == CIMQ_ROUTE_WIDE)
      return fail(CIMQ_EUNSUPPORTED, "cimq_module_forward_codes: the wide route takes no x_codes and writes no "
                                     "out_codes (cimq_module_codes_supported)");
    if (xq && !codes_qp_ok(g.lsq_qp))
      return fail(CIMQ_EUNSUPPORTED, "cimq_module_forward_codes: x_codes needs an integer lsq_qp in [1, 254] (it is %g)",
                  (double)g.lsq_qp);
    if (oq && rc.fwd == CIMQ_ROUTE_DENSE)
      return fail(CIMQ_EUNSUPPORTED, "cimq_module_forward_codes: the dense route writes no out_codes "
                                     "(cimq_module_codes_supported)");
    if (oq) {  // out_codes against every other buffer of the call whose extent the geometry gives
      const uintptr_t q0 = reinterpret_cast<uintptr_t>(oq), qn = (uintptr_t)g.M * g.O;
      auto hits = [&](const void* p, uintptr_t nb) {
        const uintptr_t p0 = reinterpret_cast<uintptr_t>(p);
        return p && p0 < q0 + qn && q0 < p0 + nb;
      };
      if (hits(out, qn * 4)) return fail(CIMQ_EINVAL, "cimq_module_forward_codes: out_codes overlaps out");
      if (hits(xq, (uintptr_t)g.Nin)) return fail(CIMQ_EINVAL, "cimq_module_forward_codes: out_codes overlaps x_codes");
      if (!xq && hits(x, (uintptr_t)g.Nin * 4)) return fail(CIMQ_EINVAL, "cimq_module_forward_codes: out_codes overlaps x");
      if (hits(ep->res, res_bytes)) return fail(CIMQ_EINVAL, "cimq_module_forward_codes: out_codes overlaps the residual");
    }
  }
  if ((!x && !xq) || !weight || !alpha_act || !alpha_weight || !binary_mask || !signed_act ||
      (!out && !(ep && ep->nofloat)) || !ctx || !ws)
    return fail(CIMQ_EINVAL, "null pointer argument");
  CIMQ_TRY(check_alpha(g, &la, alpha_cim, nullptr, false));
  if (pool) {  // what cimq_module_pool_supported answers, with its reason
    const char* why = nullptr;
    if (route_of(g).fwd != CIMQ_ROUTE_WIDE) why = "the layer is off the wide route (cimq_module_route)";
    else (void)wide_pool_ok(g, wide_plan(g), &why);
    if (why) return fail(CIMQ_EUNSUPPORTED, "cimq_module_forward_pool: %s (cimq_module_pool_supported)", why);
  }
  if (dry) return CIMQ_OK;
  const bool has_alpha = la.nbits_alpha > 0;
  const Route r = route_of(g);
  const bool q8 = stage8 && ep && x && !xq && !oq && !ep->nofloat && !ep->rvw1 && !pool && fwd8_stage_ok(g);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  uint8_t* c = reinterpret_cast<uint8_t*>(ctx);
  CtxLayout L = ctx_layout(g);
  float* scal = reinterpret_cast<float*>(wreg(g, c) + L.lsq_scal);
  {
    int nwblk;
    ModulePrep a = module_prep_args(g, x, weight, alpha_act, alpha_weight, has_alpha ? alpha_cim : nullptr,
                                    binary_mask, signed_act, c, &nwblk);
    if (beta_cim) {  // the shift ADC: beta into the thresholds, and the per-channel beta sums
      a.beta = beta_cim;
      a.npp += g.Opad;
      nwblk = prep_wblocks(a);
    }
    if (g.wbase) nwblk = 0;  // weight side prepared (cimq_module_prepare): the activation quantiser only
    if (r.actq || q8) a.nact_blocks = 0;  // the forward's row staging quantises (stage_rows_q, stage_rows_q8)
    if (a.nact_blocks + nwblk == 0) goto prepared;
    {
    const int slot = prof_begin(KID_PREP_ACT, g, s);
    ModulePrep aw = a;
    if (nwblk > 0 && has_alpha && la.nalpha > kFinishInReg && tune("WIDE_PREP", 1)) {  // wide alpha_cim: its max / min in 64 blocks first
      float* part = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(ws) + ws_layout(g).lsq_part);
      hipLaunchKernelGGL(alpha_minmax_kernel, dim3(64), dim3(256), 0, s, alpha_cim, la.nalpha, part);
      aw.amm = part;
      aw.namm = 64;
    }
    if (xq)  // (forward only; off the staging-quantiser routes, whose a.nact_blocks is 0: the bytes become slice words here)
      hipLaunchKernelGGL(prep_module_fwd_codes_kernel, dim3(a.nact_blocks + nwblk), dim3(256), 0, s, g, la, aw, xq);
    else if (g.inference)
      hipLaunchKernelGGL(prep_module_fwd_kernel, dim3(a.nact_blocks + nwblk), dim3(256), 0, s, g, la, aw);
    else
      hipLaunchKernelGGL(prep_module_kernel, dim3(a.nact_blocks + nwblk), dim3(256), 0, s, g, la, aw);
    prof_end(slot, s);
    CIMQ_TRY(check_hip("prep_module"));
    }
  }
prepared:
  const ActQ aq{x, signed_act};
  // (input codes reach the forward kernel only where its own staging reads them: elsewhere the prologue above has
  // turned them into slice words)
  Epi epk;
  if (ep && xq && !r.actq) {
    epk = *ep;
    epk.xq = nullptr;
    ep = &epk;
  }
  // (the fast forward writes NCHW, g.onchw; the dense one's P = 1: NCHW is [B, P, O])
  if (pool) return launch_wide(g, wide_plan(g), c, scal + 1, scal, out, s, &aq, ep, true);
  if (q8) return launch_fwd8_staged(g, c, scal + 1, scal, out, s, &aq, ep);
  if (r.fwd != CIMQ_ROUTE_GENERAL)
    return launch_fwd_any(g, c, scal + 1, scal, out, nullptr, nullptr, s, r.actq ? &aq : nullptr, ep);
  // general kernels write [B, P, O]; the module returns NCHW
  WsLayout W = ws_layout(g);
  float* bpo = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(ws) + W.bpo);
  CIMQ_TRY(launch_fwd_any(g, c, scal + 1, scal, bpo, nullptr, nullptr, s));
  const dim3 tgrid(std::min(cdiv((long long)g.M * g.O, 256), 8192));
  switch (fwd_mode_of(g, ep)) {  // (of codes, out_codes alone get here: x_codes were cleared above)
    case FwdMode::VIEW: hipLaunchKernelGGL(bpo_to_nchw_view_kernel, tgrid, dim3(256), 0, s, g, bpo, out, *ep); break;
    case FwdMode::CODES: hipLaunchKernelGGL(bpo_to_nchw_codes_kernel, tgrid, dim3(256), 0, s, g, bpo, out, *ep); break;
    case FwdMode::EPI: hipLaunchKernelGGL(bpo_to_nchw_epi_kernel, tgrid, dim3(256), 0, s, g, bpo, out, *ep); break;
    default: hipLaunchKernelGGL(bpo_to_nchw_kernel, tgrid, dim3(256), 0, s, g, bpo, out);
  }
  return check_hip("bpo_to_nchw");
}

int cimq_module_forward(const cimq_conv_desc* d, const cimq_lsq_desc* q, const float* x, const float* weight,
                        const float* alpha_act, const float* alpha_weight, const float* alpha_cim,
                        const int8_t* binary_mask, const float* signed_act, float* out, void* ctx, void* ws,
                        void* stream) {
  return module_forward_impl(d, q, x, weight, alpha_act, alpha_weight, alpha_cim, nullptr, binary_mask, signed_act,
                             out, ctx, ws, stream);
}

int cimq_module_route(const cimq_conv_desc* d, int* route) {
  Geo g;
  CIMQ_TRY(make_geo(d, &g));
  if (!route) return fail(CIMQ_EINVAL, "null route");
  if (g.input_kind != CIMQ_INPUT_RAW_LSQ) return fail(CIMQ_EINVAL, "module entry points take the raw activation");
  // the Function and the module entry points route a descriptor differently but share its buffers
  if (!routes_agree(g)) return fail(CIMQ_EINVAL, "internal: layouts depend on the output layout flag");
  const Route r = route_of(module_form(g));
  route[0] = r.fwd;
  route[1] = r.gx;
  route[2] = r.gw;
  return CIMQ_OK;
}

int cimq_w4a4_eval_abi(void) { return 1; }

int cimq_wide_abi(void) { return 1; }

int cimq_module_wide_plan(const cimq_conv_desc* d, int out[4]) {
  Geo g;
  CIMQ_TRY(make_geo(d, &g));
  if (!out) return fail(CIMQ_EINVAL, "null out");
  if (g.input_kind != CIMQ_INPUT_RAW_LSQ) return fail(CIMQ_EINVAL, "module entry points take the raw activation");
  g = module_form(g);
  const PlanW p = wide_plan(g);
  const bool ok = route_of(g).fwd == CIMQ_ROUTE_WIDE;
  out[0] = ok ? 1 : 0;
  out[1] = ok ? p.w.nch : 0;
  out[2] = ok ? p.groups : 0;
  out[3] = ok ? g.T : 0;
  return CIMQ_OK;
}

int cimq_module_forward_form(const cimq_conv_desc* d, int form[2]) {
  Geo g;
  CIMQ_TRY(make_geo(d, &g));
  if (!form) return fail(CIMQ_EINVAL, "null form");
  if (g.input_kind != CIMQ_INPUT_RAW_LSQ) return fail(CIMQ_EINVAL, "module entry points take the raw activation");
  const Route r = route_of(module_form(g));
  form[0] = r.cst;
  form[1] = r.actq ? 1 : 0;
  return CIMQ_OK;
}

int cimq_module_shift_supported(const cimq_conv_desc* d) {
  Geo g;
  if (make_geo(d, &g) != CIMQ_OK) return 0;
  return (g.input_kind == CIMQ_INPUT_RAW_LSQ && g.variant == VAR_SHIFT_ROUND && route_of(g).shift_stats) ? 1 : 0;
}

int cimq_module_shift_forward(const cimq_conv_desc* d, const cimq_lsq_desc* q, const float* x, const float* weight,
                              const float* alpha_act, const float* alpha_weight, const float* alpha_cim,
                              const float* beta_cim, const int8_t* binary_mask, const float* signed_act, float* out,
                              void* ctx, void* ws, void* stream) {
  if (!beta_cim || !alpha_cim) return fail(CIMQ_EINVAL, "cimq_module_shift_forward needs alpha_cim and beta_cim");
  return module_forward_impl(d, q, x, weight, alpha_act, alpha_weight, alpha_cim, beta_cim, binary_mask, signed_act,
                             out, ctx, ws, stream);
}

int cimq_module_forward_epilogue(const cimq_conv_desc* d, const cimq_lsq_desc* q, const float* x,
                                 const float* weight, const float* alpha_act, const float* alpha_weight,
                                 const float* alpha_cim, const float* beta_cim, const int8_t* binary_mask,
                                 const float* signed_act, const cimq_epilogue* epi, float* out, void* ctx, void* ws,
                                 void* stream) {
  // (the descriptor-independent refusals first, before any other argument is looked at)
  CIMQ_TRY(check_forward_only(who_epi, d));
  CIMQ_TRY(check_epilogue(who_epi, epi, alpha_cim, beta_cim));
  const Epi ep = epi_of(epi);
  return module_forward_impl(d, q, x, weight, alpha_act, alpha_weight, alpha_cim, beta_cim, binary_mask, signed_act,
                             out, ctx, ws, stream, &ep);
}

int cimq_pool_abi(void) { return 1; }

int cimq_module_pool_supported(const cimq_conv_desc* d, int* ok) {
  Geo g;
  CIMQ_TRY(make_geo(d, &g));
  if (!ok) return fail(CIMQ_EINVAL, "null ok");
  if (g.input_kind != CIMQ_INPUT_RAW_LSQ) return fail(CIMQ_EINVAL, "module entry points take the raw activation");
  g = module_form(g);
  *ok = (g.inference && route_of(g).fwd == CIMQ_ROUTE_WIDE && wide_pool_ok(g, wide_plan(g))) ? 1 : 0;
  return CIMQ_OK;
}

int cimq_module_forward_pool(const cimq_conv_desc* d, const cimq_lsq_desc* q, const float* x, const float* weight,
                             const float* alpha_act, const float* alpha_weight, const float* alpha_cim,
                             const float* beta_cim, const int8_t* binary_mask, const float* signed_act,
                             const cimq_epilogue* epi, int pool, float* out, void* ctx, void* ws, void* stream) {
  static const char who[] = "cimq_module_forward_pool";
  CIMQ_TRY(check_forward_only(who, d));
  CIMQ_TRY(check_epilogue(who, epi, alpha_cim, beta_cim));
  if (pool != 0 && pool != CIMQ_POOL_MAX2) return fail(CIMQ_EINVAL, "%s: pool must be 0 or CIMQ_POOL_MAX2 (it is %d)", who, pool);
  if (pool && beta_cim) return fail(CIMQ_EUNSUPPORTED, "%s: the shift ADC's layers run off the wide route: no pooled store", who);
  const Epi ep = epi_of(epi);
  return module_forward_impl(d, q, x, weight, alpha_act, alpha_weight, alpha_cim, beta_cim, binary_mask, signed_act,
                             out, ctx, ws, stream, &ep, false, pool);
}

int cimq_module_codes_supported(const cimq_conv_desc* d, int* in_ok, int* out_ok) {
  if (!d) return fail(CIMQ_EINVAL, "null descriptor");
  cimq_conv_desc di = *d;  // (the call takes forward-only descriptors alone: answer for that form)
  di.options |= CIMQ_OPT_INFERENCE;
  Geo g;
  CIMQ_TRY(make_geo(&di, &g));
  if (g.input_kind != CIMQ_INPUT_RAW_LSQ) return fail(CIMQ_EINVAL, "module entry points take the raw activation");
  g = module_form(g);
  const int fwd = route_of(g).fwd;
  if (in_ok) *in_ok = (codes_qp_ok(g.lsq_qp) && fwd != CIMQ_ROUTE_WIDE) ? 1 : 0;
  if (out_ok) *out_ok = (fwd == CIMQ_ROUTE_FWD5 || fwd == CIMQ_ROUTE_V3 || fwd == CIMQ_ROUTE_GENERAL) ? 1 : 0;
  return CIMQ_OK;
}

}  // extern "C"

// cimq_module_forward_codes, and one layer of cimq_net_forward: pool and stage8 (the net alone) as
// module_forward_impl's; view (the net alone) makes epi->residual a view of
// a larger tensor (Epi::rvw0 / rvw1); dry (the net's validation pass) stops before the first launch
static int forward_codes_impl(const cimq_conv_desc* d, const cimq_lsq_desc* q, const cimq_act_codes* io,
                              const float* x, const float* weight, const float* alpha_act,
                              const float* alpha_weight, const float* alpha_cim, const float* beta_cim,
                              const int8_t* binary_mask, const float* signed_act, const cimq_epilogue* epi,
                              float* out, void* ctx, void* ws, void* stream, const ResView* view = nullptr,
                              bool dry = false, int pool = 0, bool stage8 = false) {
  // (the descriptor-independent refusals first; the epilogue's are cimq_module_forward_epilogue's own)
  static const char who[] = "cimq_module_forward_codes";
  CIMQ_TRY(check_forward_only(who, d));
  if (!io) return fail(CIMQ_EINVAL, "cimq_module_forward_codes: null io");
  CIMQ_TRY(check_epilogue(who, epi, alpha_cim, beta_cim));
  if (io->flags & ~CIMQ_CODES_NO_FLOAT) return fail(CIMQ_EINVAL, "cimq_module_forward_codes: unknown flags 0x%x", io->flags);
  if (io->reserved != 0) return fail(CIMQ_EINVAL, "cimq_module_forward_codes: reserved must be 0");
  if (!io->x_codes && !io->out_codes && !io->flags) {  // no codes: cimq_module_forward_epilogue
    Epi ep = epi_of(epi);
    if (view) set_res_view(&ep, view->c0, view->cr, view->s, view->h, view->w);
    return module_forward_impl(d, q, x, weight, alpha_act, alpha_weight, alpha_cim, beta_cim, binary_mask, signed_act,
                               out, ctx, ws, stream, &ep, dry, pool, stage8);
  }
  if ((io->flags & CIMQ_CODES_NO_FLOAT) && !io->out_codes)
    return fail(CIMQ_EINVAL, "cimq_module_forward_codes: CIMQ_CODES_NO_FLOAT needs out_codes");
  if (io->out_codes) {
    if (!io->out_alpha_act) return fail(CIMQ_EINVAL, "cimq_module_forward_codes: out_codes needs out_alpha_act");
    if (!codes_qp_ok(io->out_qp))
      return fail(CIMQ_EINVAL, "cimq_module_forward_codes: out_qp must be an integer in [1, 254] (it is %g)",
                  (double)io->out_qp);
  }
  if (reinterpret_cast<uintptr_t>(io->x_codes) % 16 != 0 || reinterpret_cast<uintptr_t>(io->out_codes) % 16 != 0)
    return fail(CIMQ_EINVAL, "cimq_module_forward_codes: code buffers must be 16-byte aligned");
  Epi ep = epi_of(epi);
  ep.nofloat = (io->flags & CIMQ_CODES_NO_FLOAT) ? 1 : 0;
  ep.xq = io->x_codes;
  ep.oq = io->out_codes;
  ep.oalpha = io->out_alpha_act;
  ep.ogs = io->out_gscale_a;
  ep.oqp = io->out_qp;
  if (view) set_res_view(&ep, view->c0, view->cr, view->s, view->h, view->w);
  return module_forward_impl(d, q, x, weight, alpha_act, alpha_weight, alpha_cim, beta_cim, binary_mask, signed_act,
                             out, ctx, ws, stream, &ep, dry, pool, stage8);
}

// ---- cimq_net_*: a plan of fused conv layers, their slots and the head, run in one call ----

// what a slot holds while the plan is walked in order
struct NetSlot {
  bool has_float = false, has_codes = false;
  int B = 0, C = 0, H = 0, W = 0;
  int consumer = -1;  // the layer whose quantiser the code plane was written for
};

// One layer's call (forward_codes_impl's arguments from the plan); view: the residual as a view, or null
static int net_layer_call(const cimq_net_desc* n, int i, const float* x, void* const* sf, void* const* sc,
                          const ResView* view, void* ws, void* stream, bool dry, int pool, bool stage8) {
  const cimq_net_layer& L = n->layers[i];
  cimq_epilogue e;
  e.scale = L.scale;
  e.shift = L.shift;
  e.residual = L.res_slot >= 0 ? reinterpret_cast<const float*>(sf[L.res_slot]) : nullptr;
  e.flags = L.epi_flags;
  e.reserved = 0;
  cimq_act_codes io;
  memset(&io, 0, sizeof(io));
  const float* xin = x;
  if (L.in_slot >= 0) {
    xin = L.in_codes ? nullptr : reinterpret_cast<const float*>(sf[L.in_slot]);
    io.x_codes = L.in_codes ? reinterpret_cast<const uint8_t*>(sc[L.in_slot]) : nullptr;
  }
  if (L.out_mode & 2) {
    const cimq_net_layer& K = n->layers[L.consumer];
    io.out_codes = reinterpret_cast<uint8_t*>(sc[L.out_slot]);
    io.out_alpha_act = K.alpha_act;
    io.out_gscale_a = K.lsq->gscale_a;
    io.out_qp = K.desc->lsq_qp;
    if (!(L.out_mode & 1)) io.flags = CIMQ_CODES_NO_FLOAT;
  }
  float* out = (L.out_mode & 1) ? reinterpret_cast<float*>(sf[L.out_slot]) : nullptr;
  return forward_codes_impl(L.desc, L.lsq, &io, xin, L.weight, L.alpha_act, L.alpha_weight, L.alpha_cim, L.beta_cim,
                            L.binary_mask, L.signed_act, &e, out, L.ctx, ws, stream, view, dry, pool, stage8);
}

// The whole validation of a plan, in layer order, and with ``run`` its launches.  bufs: the caller's buffers are
// there to be checked (cimq_net_forward) -- each layer's own call is then made dry, so that every refusal it has
// comes before the first launch.  fb / cb / wsb: cimq_net_sizes' outputs (may be null).
static int net_walk(const cimq_net_desc* n, bool bufs, bool run, const float* x, void* const* sf, void* const* sc,
                    float* logits, void* ws, void* stream, size_t* fb, size_t* cb, size_t* wsb,
                    const cimq_net_ext* ext) {
  static const char who[] = "cimq_net_forward";
  if (!n) return fail(CIMQ_EINVAL, "%s: null plan", who);
  if (ext) {  // (cimq_net_*_ex: pooled layers and the flatten head; null is the plan alone)
    if (ext->head_flags & ~CIMQ_NET_HEAD_FLATTEN) return fail(CIMQ_EINVAL, "%s: ext: unknown head_flags 0x%x", who, ext->head_flags);
    if (ext->reserved[0] != 0 || ext->reserved[1] != 0 || ext->reserved[2] != 0)
      return fail(CIMQ_EINVAL, "%s: ext: reserved must be 0", who);
    for (int i = 0; ext->pool && i < n->n_layers; ++i)
      if (ext->pool[i] != 0 && ext->pool[i] != CIMQ_POOL_MAX2)
        return fail(CIMQ_EINVAL, "%s: ext: pool[%d] must be 0 or CIMQ_POOL_MAX2 (it is %d)", who, i, ext->pool[i]);
  }
  if (n->n_layers < 0 || n->n_slots < 0) return fail(CIMQ_EINVAL, "%s: negative n_layers or n_slots", who);
  if (n->n_layers == 0 && !n->head) return fail(CIMQ_EINVAL, "%s: n_layers == 0 without a head", who);
  if (n->n_layers > 0 && !n->layers) return fail(CIMQ_EINVAL, "%s: null layers", who);
  if (n->B < 1 || n->C < 1 || n->H < 1 || n->W < 1) return fail(CIMQ_EINVAL, "%s: bad input shape", who);
  auto misaligned = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 != 0; };
  if (bufs) {
    if (!x) return fail(CIMQ_EINVAL, "%s: null x", who);
    if (misaligned(x)) return fail(CIMQ_EINVAL, "%s: x must be 16-byte aligned", who);
    if (n->n_slots > 0 && (!sf || !sc)) return fail(CIMQ_EINVAL, "%s: null slot arrays", who);
    if (n->n_layers > 0 && !ws) return fail(CIMQ_EINVAL, "%s: null workspace", who);
  }
  std::vector<NetSlot> slot((size_t)n->n_slots);
  for (int k = 0; k < n->n_slots; ++k) {
    if (fb) fb[k] = 0;
    if (cb) cb[k] = 0;
  }
  size_t wsmax = 0;
  auto in_range = [&](int k) { return k >= 0 && k < n->n_slots; };
  for (int i = 0; i < n->n_layers; ++i) {
    const cimq_net_layer& L = n->layers[i];
    if (!L.desc || !L.lsq) return fail(CIMQ_EINVAL, "%s: layer %d: null descriptor", who, i);
    if (L.reserved != 0) return fail(CIMQ_EINVAL, "%s: layer %d: reserved must be 0", who, i);
    CIMQ_TRY(check_forward_only(who, L.desc));
    Geo g;
    CIMQ_TRY(make_geo(L.desc, &g));
    if (g.input_kind != CIMQ_INPUT_RAW_LSQ) return fail(CIMQ_EINVAL, "%s: layer %d: module entry points take the raw activation", who, i);
    g = module_form(g);
    if (g.variant == VAR_STOCHASTIC)
      return fail(CIMQ_EUNSUPPORTED, "%s: layer %d: a stochastic-ADC layer takes its seed per call", who, i);
    const int fwd = route_of(g).fwd;
    // the input
    if (L.in_codes != 0 && L.in_codes != 1) return fail(CIMQ_EINVAL, "%s: layer %d: in_codes must be 0 or 1", who, i);
    if (L.in_slot == -1) {
      if (L.in_codes) return fail(CIMQ_EINVAL, "%s: layer %d: the net's input x has no code plane", who, i);
      if (g.B != n->B || g.C != n->C || g.H != n->H || g.W != n->W)
        return fail(CIMQ_EINVAL, "%s: layer %d: its descriptor's input shape is not x's", who, i);
    } else {
      if (!in_range(L.in_slot)) return fail(CIMQ_EINVAL, "%s: layer %d: in_slot %d out of range", who, i, L.in_slot);
      const NetSlot& s = slot[L.in_slot];
      if (L.in_codes ? !s.has_codes : !s.has_float)
        return fail(CIMQ_EINVAL, "%s: layer %d: reads a plane of slot %d that no earlier layer wrote", who, i, L.in_slot);
      if (L.in_codes && s.consumer != i)
        return fail(CIMQ_EINVAL, "%s: layer %d: the codes in slot %d were written for layer %d", who, i, L.in_slot, s.consumer);
      if (g.B != s.B || g.C != s.C || g.H != s.H || g.W != s.W)
        return fail(CIMQ_EINVAL, "%s: layer %d: the producer's output shape [%d, %d, %d, %d] differs from its descriptor's "
                                 "input", who, i, s.B, s.C, s.H, s.W);
      if (L.in_codes && !codes_qp_ok(g.lsq_qp))
        return fail(CIMQ_EUNSUPPORTED, "%s: layer %d: x_codes needs an integer lsq_qp in [1, 254]", who, i);
      if (L.in_codes && fwd == CIMQ_ROUTE_WIDE)
        return fail(CIMQ_EUNSUPPORTED, "%s: layer %d: the wide route takes no x_codes (cimq_module_codes_supported)",
                    who, i);
    }
    // the output
    if (L.out_mode < 1 || L.out_mode > 3) return fail(CIMQ_EINVAL, "%s: layer %d: out_mode must be 1, 2 or 3", who, i);
    if (!in_range(L.out_slot)) return fail(CIMQ_EINVAL, "%s: layer %d: out_slot %d out of range", who, i, L.out_slot);
    if (L.out_slot == L.in_slot || L.out_slot == L.res_slot)
      return fail(CIMQ_EINVAL, "%s: layer %d: out_slot is its own in_slot or res_slot", who, i);
    if (L.out_mode & 2) {
      if (L.consumer <= i || L.consumer >= n->n_layers || n->layers[L.consumer].in_slot != L.out_slot)
        return fail(CIMQ_EINVAL, "%s: layer %d: consumer %d is not a later layer that reads slot %d", who, i, L.consumer,
                    L.out_slot);
      const cimq_net_layer& K = n->layers[L.consumer];
      if (!K.desc || !K.lsq) return fail(CIMQ_EINVAL, "%s: layer %d: null descriptor", who, L.consumer);
      if (fwd == CIMQ_ROUTE_DENSE)
        return fail(CIMQ_EUNSUPPORTED, "%s: layer %d: the dense route writes no out_codes (cimq_module_codes_supported)",
                    who, i);
      if (fwd == CIMQ_ROUTE_WIDE)
        return fail(CIMQ_EUNSUPPORTED, "%s: layer %d: the wide route writes no out_codes (cimq_module_codes_supported)",
                    who, i);
      if (!codes_qp_ok(K.desc->lsq_qp))
        return fail(CIMQ_EUNSUPPORTED, "%s: layer %d: its consumer %d reads no codes (an integer lsq_qp in [1, 254]; "
                                       "cimq_module_codes_supported)", who, i, L.consumer);
    }
    // the residual
    ResView view{};
    bool is_view = false;
    if (L.res_slot != -1) {
      if (!in_range(L.res_slot)) return fail(CIMQ_EINVAL, "%s: layer %d: res_slot %d out of range", who, i, L.res_slot);
      const NetSlot& s = slot[L.res_slot];
      if (!s.has_float)
        return fail(CIMQ_EINVAL, "%s: layer %d: reads a plane of slot %d that no earlier layer wrote", who, i, L.res_slot);
      const int rs = L.res_stride;
      if (rs != 1 && rs != 2) return fail(CIMQ_EINVAL, "%s: layer %d: res_stride must be 1 or 2", who, i);
      if (s.B != g.B || (s.H + rs - 1) / rs != g.Ho || (s.W + rs - 1) / rs != g.Wo)
        return fail(CIMQ_EINVAL, "%s: layer %d: the residual source [%d, %d, %d, %d] at stride %d is not the output's "
                                 "[%d, %d]", who, i, s.B, s.C, s.H, s.W, rs, g.Ho, g.Wo);
      if (L.res_c0 < 0 || L.res_c0 + s.C > g.O)
        return fail(CIMQ_EINVAL, "%s: layer %d: res_c0 %d with %d source channels leaves the %d output channels", who, i,
                    L.res_c0, s.C, g.O);
      is_view = rs == 2 || s.C != g.O;
      if (is_view) {
        if (fwd == CIMQ_ROUTE_DENSE)
          return fail(CIMQ_EUNSUPPORTED, "%s: layer %d: the dense route reads no residual view (res_stride 2 or fewer "
                                         "source channels than out_channels)", who, i);
        if (fwd == CIMQ_ROUTE_WIDE)
          return fail(CIMQ_EUNSUPPORTED, "%s: layer %d: the wide route reads no residual view (res_stride 2 or fewer "
                                         "source channels than out_channels)", who, i);
        if (fwd != CIMQ_ROUTE_GENERAL && g.Wo % 4 != 0)
          return fail(CIMQ_EUNSUPPORTED, "%s: layer %d: a residual view on the fwd5 / v3 routes needs an output width that "
                                         "is a multiple of 4 (it is %d)", who, i, g.Wo);
        if (s.C > kViewMaxDim ||s.H > kViewMaxDim || s.W > kViewMaxDim || g.O > kViewMaxDim)
          return fail(CIMQ_EUNSUPPORTED, "%s: layer %d: a residual view's dimensions must fit 15 bits", who, i);
        view = ResView{L.res_c0, s.C, rs, s.H, s.W};
      }
    }
    // a pooled layer (ext->pool): its slot holds [B, O, Ho/2, Wo/2]; its residual, checked above, has the unpooled shape
    const int pool = (ext && ext->pool) ? ext->pool[i] : 0;
    if (pool) {
      const char* why = nullptr;
      if (fwd != CIMQ_ROUTE_WIDE) why = "the layer is off the wide route (cimq_module_route)";
      else (void)wide_pool_ok(g, wide_plan(g), &why);
      if (why) return fail(CIMQ_EUNSUPPORTED, "%s: layer %d: no pooled store: %s (cimq_module_pool_supported)", who, i, why);
    }
    if (fb && (L.out_mode & 1)) fb[L.out_slot] = std::max(fb[L.out_slot], (size_t)g.M * g.O * (pool ? 1 : 4));
    if (cb && (L.out_mode & 2)) cb[L.out_slot] = std::max(cb[L.out_slot], (size_t)g.M * g.O);
    wsmax = std::max(wsmax, ws_layout(g).total);
    if (bufs) {
      auto bad = [&](const void* p) { return !p || misaligned(p); };
      if ((L.in_slot >= 0 && bad(L.in_codes ? sc[L.in_slot] : sf[L.in_slot])) || ((L.out_mode & 1) && bad(sf[L.out_slot])) ||
          ((L.out_mode & 2) && bad(sc[L.out_slot])) || (L.res_slot >= 0 && bad(sf[L.res_slot])))
        return fail(CIMQ_EINVAL, "%s: layer %d: a slot buffer it uses is null or not 16-byte aligned", who, i);
      // every refusal of the per-layer call, and with run its launches
      // (a plan given with an ext is a cimq_net_forward_ex plan: its w8a8 layers quantise in their row staging)
      CIMQ_TRY(net_layer_call(n, i, x, sf, sc, is_view ? &view : nullptr, ws, stream, !run, pool, ext != nullptr));
    }
    NetSlot& o = slot[L.out_slot];
    o.has_float = (L.out_mode & 1) != 0;
    o.has_codes = (L.out_mode & 2) != 0;
    o.consumer = o.has_codes ? L.consumer : -1;
    o.B = g.B; o.C = g.O; o.H = pool ? g.Ho / 2 : g.Ho; o.W = pool ? g.Wo / 2 : g.Wo;
  }
  if (wsb) *wsb = wsmax;
  if (const cimq_net_head* h = n->head) {
    if (h->reserved[0] != 0 || h->reserved[1] != 0) return fail(CIMQ_EINVAL, "%s: head: reserved must be 0", who);
    if (h->classes < 1) return fail(CIMQ_EINVAL, "%s: head: classes must be at least 1", who);
    if (!h->weight) return fail(CIMQ_EINVAL, "%s: head: null weight", who);
    int B = n->B, C = n->C, H = n->H, W = n->W;
    const float* src = x;
    if (h->in_slot != -1) {
      if (!in_range(h->in_slot)) return fail(CIMQ_EINVAL, "%s: head: in_slot %d out of range", who, h->in_slot);
      const NetSlot& s = slot[h->in_slot];
      if (!s.has_float) return fail(CIMQ_EINVAL, "%s: head: reads a plane of slot %d that no earlier layer wrote", who, h->in_slot);
      B = s.B; C = s.C; H = s.H; W = s.W;
      if (bufs) src = reinterpret_cast<const float*>(sf[h->in_slot]);
    }
    if (ext && (ext->head_flags & CIMQ_NET_HEAD_FLATTEN)) {  // the plane as [B, C * H * W, 1, 1]: a classifier over the flattened map
      const long long cf = (long long)C * H * W;
      if (cf > kHeadMaxC)
        return fail(CIMQ_EUNSUPPORTED, "%s: head: %lld flattened features, at most CIMQ_NET_HEAD_MAX_C (%d) fit its LDS plan",
                    who, cf, kHeadMaxC);
      C = (int)cf;
      H = W = 1;
    }
    if (C > kHeadMaxC)
      return fail(CIMQ_EUNSUPPORTED, "%s: head: %d channels, at most CIMQ_NET_HEAD_MAX_C (%d) fit its LDS plan", who, C, kHeadMaxC);
    if ((long long)H * W > 0x7fffffffLL / 4) return fail(CIMQ_EUNSUPPORTED, "%s: head: map too large", who);
    if (bufs) {
      if (!logits) return fail(CIMQ_EINVAL, "%s: null logits", who);
      if (!src || misaligned(src)) return fail(CIMQ_EINVAL, "%s: head: its input is null or not 16-byte aligned", who);
    }
    if (run) {
      hipLaunchKernelGGL(net_head_kernel, dim3(B), dim3(256), (size_t)C * 4, reinterpret_cast<hipStream_t>(stream), src, C,
                         H * W, h->classes, h->weight, h->bias, h->pooled, logits);
      CIMQ_TRY(check_hip("net_head"));
    }
  }
  return CIMQ_OK;
}

extern "C" {

int cimq_module_forward_codes(const cimq_conv_desc* d, const cimq_lsq_desc* q, const cimq_act_codes* io,
                              const float* x, const float* weight, const float* alpha_act,
                              const float* alpha_weight, const float* alpha_cim, const float* beta_cim,
                              const int8_t* binary_mask, const float* signed_act, const cimq_epilogue* epi,
                              float* out, void* ctx, void* ws, void* stream) {
  return forward_codes_impl(d, q, io, x, weight, alpha_act, alpha_weight, alpha_cim, beta_cim, binary_mask, signed_act,
                            epi, out, ctx, ws, stream);
}

int cimq_net_abi(void) { return 1; }

int cimq_net_sizes_ex(const cimq_net_desc* net, size_t* slot_float_bytes, size_t* slot_code_bytes, size_t* ws_bytes,
                      const cimq_net_ext* ext) {
  return net_walk(net, false, false, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, slot_float_bytes,
                  slot_code_bytes, ws_bytes, ext);
}

int cimq_net_forward_ex(const cimq_net_desc* net, const float* x, void* const* slot_float, void* const* slot_codes,
                        float* logits, void* ws, void* stream, const cimq_net_ext* ext) {
  // the whole plan is validated first (every layer's own call made dry): a refused plan launches nothing
  CIMQ_TRY(net_walk(net, true, false, x, slot_float, slot_codes, logits, ws, stream, nullptr, nullptr, nullptr, ext));
  return net_walk(net, true, true, x, slot_float, slot_codes, logits, ws, stream, nullptr, nullptr, nullptr, ext);
}

int cimq_net_sizes(const cimq_net_desc* net, size_t* slot_float_bytes, size_t* slot_code_bytes, size_t* ws_bytes) {
  return cimq_net_sizes_ex(net, slot_float_bytes, slot_code_bytes, ws_bytes, nullptr);
}

int cimq_net_forward(const cimq_net_desc* net, const float* x, void* const* slot_float, void* const* slot_codes,
                     float* logits, void* ws, void* stream) {
  return cimq_net_forward_ex(net, x, slot_float, slot_codes, logits, ws, stream, nullptr);
}

// one layer of cimq_module_prepare (beta null) or cimq_module_prepare_shift
struct PrepView {
  const cimq_conv_desc* desc;
  const cimq_lsq_desc* lsq;
  const float *weight, *alpha_act, *alpha_weight, *alpha_cim, *beta;
  const int8_t* binary_mask;
  void* wprep;
};

// the weight side of the layers in v, up to kPrepJobs of them per prep_weights_many_kernel launch
static int prepare_run(const std::vector<PrepView>& v, bool shift, hipStream_t s) {
  const int n = (int)v.size();
  PrepPack pk;
  memset(&pk, 0, sizeof(pk));
  int grid = 0;
  for (int i = 0; i < n; ++i) {
    const PrepView& it = v[i];
    Geo g;
    LsqArgs la;
    if (!it.lsq) return fail(CIMQ_EINVAL, "item %d: null LSQ descriptor", i);
    cimq_lsq_desc q = *it.lsq;
    q.flags = 0;
    q.wprep = it.wprep;
    CIMQ_TRY(module_geo(it.desc, &q, &g, &la, shift));
    if (!it.weight || !it.alpha_act || !it.alpha_weight || !it.binary_mask || !it.wprep)
      return fail(CIMQ_EINVAL, "item %d: null pointer argument", i);
    CIMQ_TRY(check_alpha(g, &la, it.alpha_cim, nullptr, false));
    PrepJob& j = pk.job[pk.n];
    j.g = g;
    j.q = la;
    j.a = module_prep_args(g, nullptr, it.weight, it.alpha_act, it.alpha_weight, la.nbits_alpha ? it.alpha_cim : nullptr,
                           it.binary_mask, nullptr, nullptr, &j.nwblk);
    if (it.beta) {  // the shift ADC: beta into the thresholds, and the per-channel beta sums (as module_forward_impl)
      j.a.beta = it.beta;
      j.a.npp += g.Opad;
      j.nwblk = prep_wblocks(j.a);
    }
    j.a.nact_blocks = 0;
    pk.blk0[pk.n] = grid;
    grid += j.nwblk;
    ++pk.n;
    if (pk.n == kPrepJobs || i == n - 1) {
      pk.blk0[pk.n] = grid;
      hipLaunchKernelGGL(prep_weights_many_kernel, dim3(grid), dim3(256), 0, s, pk);
      CIMQ_TRY(check_hip("prep_weights_many"));
      memset(&pk, 0, sizeof(pk));
      grid = 0;
    }
  }
  return CIMQ_OK;
}

static int module_backward_impl(const cimq_conv_desc* d, const cimq_lsq_desc* q, const float* grad_out,
                                const float* x, const float* weight, const float* alpha_act,
                                const float* alpha_weight, const float* alpha_cim, const int8_t* binary_mask,
                                const float* signed_act, const void* ctx, float* grad_x, float* grad_weight,
                                float* grad_alpha_act, float* grad_alpha_weight, float* grad_alpha_cim, void* ws,
                                Pending* pend, void* stream) {
  CIMQ_TRY(refuse_inference(d, "cimq_module_backward"));
  Geo g;
  LsqArgs la;
  CIMQ_TRY(module_geo(d, q, &g, &la));
  (void)alpha_act; (void)alpha_weight; (void)binary_mask;
  if (!grad_out || !x || !weight || !signed_act || !ctx || !grad_x || !grad_weight || !grad_alpha_act ||
      !grad_alpha_weight || !ws)
    return fail(CIMQ_EINVAL, "null pointer argument");
  CIMQ_TRY(check_alpha(g, &la, alpha_cim, grad_alpha_cim));
  const Route r = route_of(g);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint8_t* c = reinterpret_cast<const uint8_t*>(ctx);
  uint8_t* w = reinterpret_cast<uint8_t*>(ws);
  const float* scal = reinterpret_cast<const float*>(wreg(g, c) + ctx_layout(g).lsq_scal);
  const float* sa = scal;
  const float* sw = scal + 1;
  const float* gsrc = grad_out;
  // the general backward reads [B, P, O] grad_out, also behind the fast forward (a v3 layer off the v7 plan, e.g.
  // w4a4); the fast kernels read NCHW (g.onchw), and the dense path's P = 1
  if (r.gx == CIMQ_ROUTE_GENERAL) {
    float* bpo = reinterpret_cast<float*>(w + ws_layout(g).bpo);
    hipLaunchKernelGGL(nchw_to_bpo_kernel, dim3(std::min(cdiv((long long)g.M * g.O, 256), 8192)), dim3(256), 0, s,
                       g, grad_out, bpo);
    CIMQ_TRY(check_hip("nchw_to_bpo"));
    gsrc = bpo;
  }
  const bool defer = (q->flags & CIMQ_LSQ_DEFER_GW) && r.gw_own;
  CIMQ_TRY(dispatch_bwd_any(g, c, sw, sa, signed_act, gsrc, x, grad_x, w, s, defer ? 1 : 3));
  // the act-LSQ partials: fused into the fast grad_x kernel, a separate pass otherwise (the epilogue sums them)
  CIMQ_TRY(launch_act_lsq(g, x, sa, grad_x, w, nullptr, s));
  if (pend) {
    // the epilogue joins the pending ones: cimq_pending_flush (or a full list, or a layer whose
    // gradient buffers a pending one writes) launches them all, packed.  Until then this layer's
    // ws (its grad_w slabs: B per-image slabs on the fused / first-conv paths, ~37.7 MB for a
    // 64-channel ResNet-20 layer at B = 256) stays in use: the chain's peak memory is up to
    // kPendingJobs workspaces (cimq.h states it; bench.Trainer flushes per segment at world > 1)
    const TailLaunch j = tail_job(g, la, q, c, w, weight, alpha_cim, grad_weight, grad_alpha_act, grad_alpha_weight,
                                  grad_alpha_cim, 0, true);
    if (pend->magic == kPendingMagic && (pend->n == kPendingJobs || pending_overlaps(pend, j.a)))
      CIMQ_TRY(pending_run(pend, s));
    if (pend->magic != kPendingMagic) pend->n = 0;
    pend->nblk[pend->n] = j.tail_blocks;
    pend->job[pend->n] = tail_job_of(j);
    ++pend->n;
    pend->magic = kPendingMagic;
    return CIMQ_OK;
  }
  // the caller runs cimq_module_backward_tail / _params
  if (q->flags & (CIMQ_LSQ_SKIP_TAIL | CIMQ_LSQ_DEFER_GW)) return CIMQ_OK;
  return module_tail(g, la, q, c, w, weight, alpha_cim, grad_weight, grad_alpha_act, grad_alpha_weight,
                     grad_alpha_cim, s);
}

int cimq_module_backward(const cimq_conv_desc* d, const cimq_lsq_desc* q, const float* grad_out, const float* x,
                         const float* weight, const float* alpha_act, const float* alpha_weight,
                         const float* alpha_cim, const int8_t* binary_mask, const float* signed_act,
                         const void* ctx, float* grad_x, float* grad_weight, float* grad_alpha_act,
                         float* grad_alpha_weight, float* grad_alpha_cim, void* ws, void* stream) {
  return module_backward_impl(d, q, grad_out, x, weight, alpha_act, alpha_weight, alpha_cim, binary_mask, signed_act,
                              ctx, grad_x, grad_weight, grad_alpha_act, grad_alpha_weight, grad_alpha_cim, ws,
                              nullptr, stream);
}

int cimq_module_backward_chain(const cimq_conv_desc* d, const cimq_lsq_desc* q, const float* grad_out,
                               const float* x, const float* weight, const float* alpha_act,
                               const float* alpha_weight, const float* alpha_cim, const int8_t* binary_mask,
                               const float* signed_act, const void* ctx, float* grad_x, float* grad_weight,
                               float* grad_alpha_act, float* grad_alpha_weight, float* grad_alpha_cim, void* ws,
                               cimq_pending* pending, void* stream) {
  CIMQ_TRY(refuse_inference(d, "cimq_module_backward_chain"));
  if (!pending) return fail(CIMQ_EINVAL, "null cimq_pending");
  Pending* pd = reinterpret_cast<Pending*>(pending);
  if (pd->magic != 0 && pd->magic != kPendingMagic) return fail(CIMQ_EINVAL, "cimq_pending not initialised (zero it)");
  if (q && (q->flags & (CIMQ_LSQ_SKIP_TAIL | CIMQ_LSQ_DEFER_GW)))
    return fail(CIMQ_EINVAL, "CIMQ_LSQ_SKIP_TAIL / _DEFER_GW with the chained backward");
  return module_backward_impl(d, q, grad_out, x, weight, alpha_act, alpha_weight, alpha_cim, binary_mask, signed_act,
                              ctx, grad_x, grad_weight, grad_alpha_act, grad_alpha_weight, grad_alpha_cim, ws, pd,
                              stream);
}

int cimq_pending_jobs(const cimq_pending* pending) {
  const Pending* pd = reinterpret_cast<const Pending*>(pending);
  return (pd && pd->magic == kPendingMagic) ? pd->n : 0;
}

int cimq_pending_flush(cimq_pending* pending, void* stream) {
  if (!pending) return fail(CIMQ_EINVAL, "null cimq_pending");
  Pending* pd = reinterpret_cast<Pending*>(pending);
  if (pd->magic != 0 && pd->magic != kPendingMagic) return fail(CIMQ_EINVAL, "cimq_pending not initialised (zero it)");
  return pending_run(pd, reinterpret_cast<hipStream_t>(stream));
}

int cimq_module_backward_tail(const cimq_conv_desc* d, const cimq_lsq_desc* q, const float* weight,
                              const float* alpha_cim, const void* ctx, float* grad_weight, float* grad_alpha_act,
                              float* grad_alpha_weight, float* grad_alpha_cim, void* ws, void* stream) {
  CIMQ_TRY(refuse_inference(d, "cimq_module_backward_tail"));
  Geo g;
  LsqArgs la;
  CIMQ_TRY(module_geo(d, q, &g, &la));
  if (!weight || !ctx || !grad_weight || !grad_alpha_act || !grad_alpha_weight || !ws)
    return fail(CIMQ_EINVAL, "null pointer argument");
  CIMQ_TRY(check_alpha(g, &la, alpha_cim, grad_alpha_cim));
  return module_tail(g, la, q, reinterpret_cast<const uint8_t*>(ctx), reinterpret_cast<uint8_t*>(ws), weight,
                     alpha_cim, grad_weight, grad_alpha_act, grad_alpha_weight, grad_alpha_cim,
                     reinterpret_cast<hipStream_t>(stream));
}

int cimq_module_backward_params(const cimq_conv_desc* d, const cimq_lsq_desc* q, const float* grad_out,
                                const float* weight, const float* alpha_cim, const void* ctx, float* grad_weight,
                                float* grad_alpha_act, float* grad_alpha_weight, float* grad_alpha_cim, void* ws,
                                void* stream) {
  CIMQ_TRY(refuse_inference(d, "cimq_module_backward_params"));
  Geo g;
  LsqArgs la;
  CIMQ_TRY(module_geo(d, q, &g, &la));
  if (!(q->flags & CIMQ_LSQ_DEFER_GW)) return fail(CIMQ_EINVAL, "cimq_module_backward_params needs CIMQ_LSQ_DEFER_GW");
  if (!grad_out || !weight || !ctx || !grad_weight || !grad_alpha_act || !grad_alpha_weight || !ws)
    return fail(CIMQ_EINVAL, "null pointer argument");
  CIMQ_TRY(check_alpha(g, &la, alpha_cim, grad_alpha_cim));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint8_t* c = reinterpret_cast<const uint8_t*>(ctx);
  uint8_t* w = reinterpret_cast<uint8_t*>(ws);
  if (route_of(g).gw_own) {
    // the grad_w kernel cimq_module_backward left out (grad_out NCHW, as the v7 path reads it there)
    const float* scal = reinterpret_cast<const float*>(wreg(g, c) + ctx_layout(g).lsq_scal);
    CIMQ_TRY(dispatch_bwd_any(g, c, scal + 1, scal, nullptr, grad_out, nullptr, nullptr, w, s, 2));
  }
  return module_tail(g, la, q, c, w, weight, alpha_cim, grad_weight, grad_alpha_act, grad_alpha_weight,
                     grad_alpha_cim, s);
}

int cimq_module_shift_backward(const cimq_conv_desc* d, const cimq_lsq_desc* q, const float* grad_out,
                               const float* x, const float* weight, const float* alpha_act,
                               const float* alpha_weight, const float* alpha_cim, const float* beta_cim,
                               const int8_t* binary_mask, const float* signed_act, const void* ctx, float* grad_x,
                               float* grad_weight, float* grad_alpha_act, float* grad_alpha_weight,
                               float* grad_alpha_cim, float* grad_beta_cim, void* ws, void* stream) {
  CIMQ_TRY(refuse_inference(d, "cimq_module_shift_backward"));
  Geo g;
  LsqArgs la;
  CIMQ_TRY(module_geo(d, q, &g, &la, true));
  (void)alpha_act; (void)alpha_weight; (void)beta_cim;
  if (!grad_out || !x || !weight || !alpha_cim || !binary_mask || !signed_act || !ctx || !grad_x || !grad_weight ||
      !grad_alpha_act || !grad_alpha_weight || !grad_alpha_cim || !grad_beta_cim || !ws)
    return fail(CIMQ_EINVAL, "null pointer argument");
  if (la.nbits_alpha == 0) return fail(CIMQ_EINVAL, "the shift ADC needs alpha_cim (nbits_alpha > 0)");
  if (q->flags & (CIMQ_LSQ_SKIP_TAIL | CIMQ_LSQ_DEFER_GW))
    return fail(CIMQ_EINVAL, "CIMQ_LSQ_SKIP_TAIL / _DEFER_GW with cimq_module_shift_backward");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint8_t* c = reinterpret_cast<const uint8_t*>(ctx);
  uint8_t* w = reinterpret_cast<uint8_t*>(ws);
  WsLayout W = ws_layout(g);
  const float* scal = reinterpret_cast<const float*>(wreg(g, c) + ctx_layout(g).lsq_scal);
  // (module_geo: a v7-plan layer, whose grad_x kernel leaves the act-LSQ partials)
  CIMQ_TRY(dispatch_bwd_any(g, c, scal + 1, scal, signed_act, grad_out, x, grad_x, w, s));
  // d loss / d alpha_q and grad_beta (scale_shift.py:488-501) from the statistics kernel, then the
  // module epilogue (grad_w + weight-LSQ backward, alpha_cim's quantiser, the step sizes) from there
  CIMQ_TRY(launch_shift_stats(g, c, scal + 1, scal, grad_out, binary_mask, w, reinterpret_cast<float*>(w + W.gaq),
                              grad_beta_cim, s, (q->flags & CIMQ_LSQ_ACCUMULATE_GRADS) ? 1 : 0));
  return module_tail(g, la, q, c, w, weight, alpha_cim, grad_weight, grad_alpha_act, grad_alpha_weight,
                     grad_alpha_cim, s, 1);
}

int cimq_module_prepare(int n, const cimq_prepare_item* items, void* stream) {
  if (n < 0 || (n > 0 && !items)) return fail(CIMQ_EINVAL, "bad prepare item list");
  std::vector<PrepView> v((size_t)n);
  for (int i = 0; i < n; ++i) {
    const cimq_prepare_item& it = items[i];
    v[i] = PrepView{it.desc, it.lsq, it.weight, it.alpha_act, it.alpha_weight, it.alpha_cim, nullptr, it.binary_mask, it.wprep};
  }
  return prepare_run(v, false, reinterpret_cast<hipStream_t>(stream));
}

int cimq_shift_prepare_abi(void) { return 1; }

int cimq_module_prepare_shift(int n, const cimq_prepare_shift_item* items, void* stream) {
  static const char who[] = "cimq_module_prepare_shift";
  if (n < 0 || (n > 0 && !items)) return fail(CIMQ_EINVAL, "bad prepare item list");
  std::vector<PrepView> v((size_t)n);
  // (every refusal of the call's own before the first launch)
  for (int i = 0; i < n; ++i) {
    const cimq_prepare_shift_item& it = items[i];
    if (!it.beta_cim || !it.alpha_cim) return fail(CIMQ_EINVAL, "%s: item %d: needs alpha_cim and beta_cim", who, i);
    if (it.reserved[0] != 0 || it.reserved[1] != 0) return fail(CIMQ_EINVAL, "%s: item %d: reserved must be 0", who, i);
    if (!it.desc) return fail(CIMQ_EINVAL, "%s: item %d: null descriptor", who, i);
    if (!(it.desc->options & CIMQ_OPT_INFERENCE))
      return fail(CIMQ_EINVAL, "%s: item %d: a CIMQ_OPT_INFERENCE descriptor only (the shift backward reads nothing "
                               "prepared)", who, i);
    if (!cimq_module_shift_supported(it.desc))
      return fail(CIMQ_EUNSUPPORTED, "%s: item %d: not a layer of the fused shift path (cimq_module_shift_supported)", who, i);
    v[i] = PrepView{it.desc, it.lsq, it.weight, it.alpha_act, it.alpha_weight, it.alpha_cim, it.beta_cim, it.binary_mask,
                    it.wprep};
  }
  return prepare_run(v, true, reinterpret_cast<hipStream_t>(stream));
}

int cimq_alpha_init(const cimq_conv_desc* d, const float* x, const float* w_q, const float* sa,
                    const float* sw, const int8_t* binary_mask, const float* signed_act,
                    float* alpha_init, void* ctx, void* ws, void* stream) {
  CIMQ_TRY(refuse_inference(d, "cimq_alpha_init"));
  Geo g;
  CIMQ_TRY(make_geo(d, &g));
  if (!x || !w_q || !sa || !sw || !binary_mask || !signed_act || !alpha_init || !ctx || !ws)
    return fail(CIMQ_EINVAL, "null pointer argument");
  if (!(g.mode == ADC_SIGN || g.mode == ADC_TERNARY))
    return fail(CIMQ_EINVAL, "alpha_cim exists only for adc_bits 1 / 1.5");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  uint8_t* c = reinterpret_cast<uint8_t*>(ctx);
  uint8_t* w = reinterpret_cast<uint8_t*>(ws);
  // the init path slices activations unsigned (lsq.py:51); the fused-LSQ codes are never
  // negative there, so the signed and unsigned slicings coincide
  CIMQ_TRY(prep_all(g, x, w_q, sa, sw, nullptr, binary_mask, signed_act, c, s, false, false));
  {
    Params pp = params_of(g, c);
    if (hipMemsetAsync(pp.flags, 0, 16, s) != hipSuccess) return fail(CIMQ_EHIP, "memset flags");
  }
  CIMQ_TRY(launch_alpha_init_sums(g, c, sw, sa, signed_act, w, s));
  return launch_reduce_galpha(g, c, w, 0.f, 1, sw, sa, alpha_init, s);
}

// dist.FlatSGD's update: four elements per thread (the flat buffers are 256-B aligned torch
// allocations), the last n % 4 by thread 0 of block 0
__global__ __launch_bounds__(256) void flat_sgd_kernel(long long n, float* __restrict__ p, float* __restrict__ g,
                                                       float* __restrict__ buf, const float* __restrict__ wd, float lr,
                                                       float mom, int first, int zero_grad) {
  auto upd = [&](float pv, float gv, float bv, float w, float& po, float& bo) {
    const float d = gv + w * pv;
    bo = first ? d : mom * bv + d;
    po = pv - lr * bo;
  };
  const long long n4 = n >> 2;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n4; t += (long long)gridDim.x * blockDim.x) {
    const float4 pv = reinterpret_cast<const float4*>(p)[t], gv = reinterpret_cast<const float4*>(g)[t];
    const float4 wv = reinterpret_cast<const float4*>(wd)[t];
    const float4 bv = first ? make_float4(0.f, 0.f, 0.f, 0.f) : reinterpret_cast<const float4*>(buf)[t];
    float4 po, bo;
    upd(pv.x, gv.x, bv.x, wv.x, po.x, bo.x);
    upd(pv.y, gv.y, bv.y, wv.y, po.y, bo.y);
    upd(pv.z, gv.z, bv.z, wv.z, po.z, bo.z);
    upd(pv.w, gv.w, bv.w, wv.w, po.w, bo.w);
    reinterpret_cast<float4*>(p)[t] = po;
    reinterpret_cast<float4*>(buf)[t] = bo;
    if (zero_grad) reinterpret_cast<float4*>(g)[t] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (long long e = n4 << 2; e < n; ++e) {
      upd(p[e], g[e], first ? 0.f : buf[e], wd[e], p[e], buf[e]);
      if (zero_grad) g[e] = 0.f;
    }
}

int cimq_flat_sgd(long long n, float* param, float* grad, float* buf, const float* wd, float lr, float momentum,
                  int first, int zero_grad, void* stream) {
  if (n < 0) return fail(CIMQ_EINVAL, "negative element count");
  if (n == 0) return CIMQ_OK;
  if (!param || !grad || !buf || !wd) return fail(CIMQ_EINVAL, "null pointer argument");
  for (const void* q : {(const void*)param, (const void*)grad, (const void*)buf, (const void*)wd})
    if (reinterpret_cast<uintptr_t>(q) % 16 != 0) return fail(CIMQ_EINVAL, "cimq_flat_sgd: buffers must be 16-byte aligned");
  const long long n4 = n >> 2;
  const int grid = (int)std::max<long long>(1, std::min<long long>(cdiv(n4, 256), 2048));
  hipLaunchKernelGGL(flat_sgd_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), n, param, grad,
                     buf, wd, lr, momentum, first ? 1 : 0, zero_grad ? 1 : 0);
  return check_hip("flat_sgd");
}

int cimq_profile_start(int kernel_id, int max_launches) {
  Profiler& p = prof();
  std::lock_guard<std::mutex> lk(p.mu);
  if (p.ev) return fail(CIMQ_EINVAL, "profiler already running");
  if (kernel_id < KID_FWD || kernel_id > KID_LAST || max_launches <= 0)
    return fail(CIMQ_EINVAL, "bad profiler arguments");
  p.ev = new hipEvent_t[2 * (size_t)max_launches];
  p.lb = new double[(size_t)max_launches];
  p.lf = new double[(size_t)max_launches];
  p.lm = new double[(size_t)max_launches];
  for (int i = 0; i < 2 * max_launches; ++i) {
    if (hipEventCreate(&p.ev[i]) != hipSuccess) {
      for (int k = 0; k < i; ++k) (void)hipEventDestroy(p.ev[k]);
      delete[] p.ev;
      delete[] p.lb;
      delete[] p.lf;
      delete[] p.lm;
      p.ev = nullptr;
      p.lb = p.lf = p.lm = nullptr;
      return fail(CIMQ_EHIP, "hipEventCreate");
    }
  }
  p.kid = kernel_id;
  p.cap = max_launches;
  p.n = 0;
  p.bytes = p.flops = 0;
  return CIMQ_OK;
}

int cimq_profile_read(int cap, double* ms, double* algo_bytes, double* algo_flops, double* mfma_ops, int* launches) {
  Profiler& p = prof();
  std::lock_guard<std::mutex> lk(p.mu);
  if (!p.ev) return fail(CIMQ_EINVAL, "profiler not running");
  if (cap < 0 || (cap > 0 && (!ms || !algo_bytes || !algo_flops || !mfma_ops))) return fail(CIMQ_EINVAL, "bad buffers");
  const int n = std::min(cap, p.n);
  for (int i = 0; i < n; ++i) {
    float t = 0;
    if (hipEventSynchronize(p.ev[2 * i + 1]) != hipSuccess || hipEventElapsedTime(&t, p.ev[2 * i], p.ev[2 * i + 1]) != hipSuccess)
      return fail(CIMQ_EHIP, "hipEventElapsedTime");
    ms[i] = t;
    algo_bytes[i] = p.lb[i];
    algo_flops[i] = p.lf[i];
    mfma_ops[i] = p.lm[i];
  }
  if (launches) *launches = p.n;
  return CIMQ_OK;
}

int cimq_profile_stop(double* total_ms, int* launches, double* algo_bytes, double* algo_flops) {
  Profiler& p = prof();
  std::lock_guard<std::mutex> lk(p.mu);
  if (!p.ev) return fail(CIMQ_EINVAL, "profiler not running");
  double tot = 0;
  int rc = CIMQ_OK;
  for (int i = 0; i < p.n; ++i) {
    float ms = 0;
    if (hipEventSynchronize(p.ev[2 * i + 1]) != hipSuccess ||
        hipEventElapsedTime(&ms, p.ev[2 * i], p.ev[2 * i + 1]) != hipSuccess) {
      rc = fail(CIMQ_EHIP, "hipEventElapsedTime");
      break;
    }
    tot += ms;
  }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = p.n;
  if (algo_bytes) *algo_bytes = p.bytes;
  if (algo_flops) *algo_flops = p.flops;
  for (int i = 0; i < 2 * p.cap; ++i) (void)hipEventDestroy(p.ev[i]);
  delete[] p.ev;
  delete[] p.lb;
  delete[] p.lf;
  delete[] p.lm;
  p.ev = nullptr;
  p.lb = p.lf = p.lm = nullptr;
  p.kid = KID_NONE;
  p.cap = p.n = 0;
  return rc;
}

}  // extern "C"
