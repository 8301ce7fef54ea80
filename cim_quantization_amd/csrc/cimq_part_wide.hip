// cimq_part_wide.hip -- launch of the channel-chunked module forward (wide_plan, CIMQ_ROUTE_WIDE) and its
// explicit instances.  Own translation unit of libcimq.so.
#include "cimq_host.h"
#include "cimq_wide.hip"

namespace cimq {

using WideKern = void (*)(Geo, V3, WideP, const uint8_t*, const v4i*, Params, const float*, const float*, float*,
                          const float*, const float*, Epi);

// the instance of one (K-steps, mode) for a slice count: 2 / 3 / 4 at compile time (1-bit slices), 0 at run time
template <int KS, FwdMode M>
WideKern wide_kernel(int cst) {
  switch (cst) {
    case 2: return cim_fwd_wide_kernel<KS, 2, M>;
    case 3: return cim_fwd_wide_kernel<KS, 3, M>;
    case 4: return cim_fwd_wide_kernel<KS, 4, M>;
    default: return cim_fwd_wide_kernel<KS, 0, M>;
  }
}
template <int KS>
WideKern wide_kernel(FwdMode m, int cst) {
  switch (m) {
    case FwdMode::TRAIN: return wide_kernel<KS, FwdMode::TRAIN>(cst);
    case FwdMode::INFER: return wide_kernel<KS, FwdMode::INFER>(cst);
    case FwdMode::EPI: return wide_kernel<KS, FwdMode::EPI>(cst);
    default: return nullptr;  // codes and views: refused where the call is checked (module_forward_impl)
  }
}

// the pooled-store instances (POOL): the epilogue mode alone, the same eight (K-steps, slice count) forms
template <int KS>
WideKern wide_pool_kernel(int cst) {
  switch (cst) {
    case 2: return cim_fwd_wide_kernel<KS, 2, FwdMode::EPI, true>;
    case 3: return cim_fwd_wide_kernel<KS, 3, FwdMode::EPI, true>;
    case 4: return cim_fwd_wide_kernel<KS, 4, FwdMode::EPI, true>;
    default: return cim_fwd_wide_kernel<KS, 0, FwdMode::EPI, true>;
  }
}

int launch_wide(const Geo& g, const PlanW& p, uint8_t* ctx, const float* sw, const float* sa, float* out,
                hipStream_t s, const ActQ* aq, const Epi* ep, bool pool) {
  if (!p.ok || !g.onchw) return fail(CIMQ_EINVAL, "internal: cim_fwd_wide off its plan");
  const FwdMode m = fwd_mode_of(g, ep);
  // a forward-only call reads fp32 x (Route::actq), a training call the prologue's slice words
  if ((m != FwdMode::TRAIN) != (aq != nullptr) || (m != FwdMode::TRAIN && !g.inference))
    return fail(CIMQ_EINVAL, "internal: cim_fwd_wide's input form off its mode");
  // (out is [B, O, Ho/2, Wo/2] then: module_forward_impl has checked wide_pool_ok)
  if (pool && (m != FwdMode::EPI || !wide_pool_ok(g, p)))
    return fail(CIMQ_EINVAL, "internal: cim_fwd_wide's pooled store off its plan");
  WideKern kern = pool ? (g.KS == 1 ? wide_pool_kernel<1>(wide_cst(g)) : wide_pool_kernel<2>(wide_cst(g)))
                       : (g.KS == 1 ? wide_kernel<1>(m, wide_cst(g)) : wide_kernel<2>(m, wide_cst(g)));
  if (!kern) return fail(CIMQ_EUNSUPPORTED, "the wide route takes no activation codes and no residual view");
  CtxLayout L = ctx_layout(g);
  CIMQ_TRY(set_lds(kern, p.lds));
  // grid: m-tiles on a grid-stride loop, about four workgroups per CU over the output groups
  dim3 grid(std::min(p.v.nmt, std::max(64, tune("WIDE_GRID", 1024) / p.groups)), p.groups);
  const int slot = prof_begin(KID_FWD, g, s);
  hipLaunchKernelGGL(kern, grid, dim3(256), p.lds, s, g, p.v, p.w, ctx + L.xcode,
                     reinterpret_cast<const v4i*>(wreg(g, ctx) + L.wfrag), params_of(g, ctx), sw, sa, out,
                     aq ? aq->x : nullptr, aq ? aq->signed_act : nullptr, ep ? *ep : Epi{});
  prof_end(slot, s);
  return check_hip("cim_fwd_wide");
}

}  // namespace cimq
