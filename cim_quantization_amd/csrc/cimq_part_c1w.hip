// cimq_part_c1w.hip -- launch of the wide first conv's recompute backward under CIMQ_OPT_WIDE_BWD (c1w_plan,
// CIMQ_ROUTE_C1W): cim_bwd_c1w_kernel (= cim_bwd_c1_kernel<true, true>) over (image, output-block group) and, where an image has several
// groups, c1w_fold_kernel over the images.  Own translation unit of libcimq.so, compiled without packed fp32
// instructions (build.py); cimq_part_fused.hip, with its own flags, holds the one-block instances of the same kernel.
#include "cimq_host.h"
#include "cimq_c1w.hip"

namespace cimq {

int launch_c1w(const Geo& g, const PlanC1W& p, const uint8_t* ctx, const float* sw, const float* sa, const float* gout,
               const float* x, float* gx, uint8_t* ws, hipStream_t s) {
  if (!p.ok || g.inference || route_of(g).gx != CIMQ_ROUTE_C1W)
    return fail(CIMQ_EINVAL, "internal: the wide first-conv backward off its plan");
  if (!x || !gx) return fail(CIMQ_EINVAL, "internal: the wide first-conv backward without x / grad_x");
  CtxLayout L = ctx_layout(g);
  WsLayout W = ws_layout(g);
  Params pp = params_of(g, const_cast<uint8_t*>(ctx));
  // the group partials: the unfolded-grad_x region, M * K floats = 9 partials of Nin = C * M
  if (p.v.groups > 1 && (size_t)p.v.groups * (size_t)g.Nin > (size_t)g.M * g.K)
    return fail(CIMQ_EINVAL, "internal: the group partials do not fit the workspace");
  float* part = reinterpret_cast<float*>(ws + W.gxu);
  float* gsa = reinterpret_cast<float*>(ws + W.lsq_part);
  CIMQ_TRY(set_lds(cim_bwd_c1w_kernel, p.v.c.lds));
  const int slot = prof_begin(KID_FUSED, g, s);
  hipLaunchKernelGGL(cim_bwd_c1w_kernel, dim3(g.B, p.v.groups), dim3(512), p.v.c.lds, s, g, p.v, ctx + L.xcode,
                     ctx + L.xhat, reinterpret_cast<const v4i*>(wreg(g, ctx) + L.wfrag),
                     reinterpret_cast<const v4i*>(wreg(g, ctx) + L.wcy), pp, sw, sa, gout, x, gx, part,
                     reinterpret_cast<float*>(ws + W.gw_slab), reinterpret_cast<float*>(ws + W.ga_slab), gsa);
  prof_end(slot, s);
  CIMQ_TRY(check_hip("cim_bwd_c1w"));
  if (p.v.groups > 1) {
    hipLaunchKernelGGL(c1w_fold_kernel, dim3(g.B), dim3(256), 0, s, g, p.v.groups, part, sw, sa, x, gx, gsa);
    CIMQ_TRY(check_hip("c1w_fold"));
  }
  return CIMQ_OK;
}

}  // namespace cimq
