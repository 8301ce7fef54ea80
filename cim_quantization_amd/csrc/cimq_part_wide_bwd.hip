// cimq_part_wide_bwd.hip -- launches of a wide layer's training path under CIMQ_OPT_WIDE_BWD (wide_bwd_plan,
// CIMQ_ROUTE_WIDE_BWD): cim_fwd_wide_state_kernel, cim_bwd_gx_wide_kernel and cim_bwd_gw_wide_kernel.  Own
// translation unit of libcimq.so, compiled without packed fp32 instructions (build.py); cimq_part_wide.hip, its
// flags and its instances stay what they were.
#include "cimq_host.h"
#include "cimq_wide_state.hip"
#include "cimq_wide_bwd.hip"

namespace cimq {

using WideStateKern = void (*)(Geo, V3, WideP, const uint8_t*, const v4i*, Params, const float*, const float*, float*,
                               uint8_t*);

template <int KS>
static WideStateKern wide_state_kernel(int cst) {
  switch (cst) {
    case 2: return cim_fwd_wide_state_kernel<KS, 2>;
    case 3: return cim_fwd_wide_state_kernel<KS, 3>;
    case 4: return cim_fwd_wide_state_kernel<KS, 4>;
    default: return nullptr;
  }
}

int launch_wide_state(const Geo& g, const PlanW& p, uint8_t* ctx, const float* sw, const float* sa, float* out,
                      hipStream_t s) {
  const Route r = route_of(g);
  if (!p.ok || !g.onchw || g.inference || r.gx != CIMQ_ROUTE_WIDE_BWD)
    return fail(CIMQ_EINVAL, "internal: cim_fwd_wide_state off its plan");
  WideStateKern kern = g.KS == 1 ? wide_state_kernel<1>(wide_cst(g)) : wide_state_kernel<2>(wide_cst(g));
  if (!kern) return fail(CIMQ_EINVAL, "internal: no state instance of this slice count");
  CtxLayout L = ctx_layout(g);
  CIMQ_TRY(set_lds(kern, p.lds));
  dim3 grid(std::min(p.v.nmt, std::max(64, tune("WIDE_GRID", 1024) / p.groups)), p.groups);
  const int slot = prof_begin(KID_FWD, g, s);
  hipLaunchKernelGGL(kern, grid, dim3(256), p.lds, s, g, p.v, p.w, ctx + L.xcode,
                     reinterpret_cast<const v4i*>(wreg(g, ctx) + L.wfrag), params_of(g, ctx), sw, sa, out,
                     ctx + L.st);
  prof_end(slot, s);
  return check_hip("cim_fwd_wide_state");
}

template <int NB>
static int launch_wide_bwd_n(const Geo& g, const PlanWB& p, const uint8_t* ctx, const float* sw, const float* sa,
                             const float* gout, const float* x, float* gx, uint8_t* ws, hipStream_t s, int parts) {
  CtxLayout L = ctx_layout(g);
  WsLayout W = ws_layout(g);
  Params pp = params_of(g, const_cast<uint8_t*>(ctx));
  const uint32_t* st = reinterpret_cast<const uint32_t*>(ctx + L.st);
  if (parts & 1) {
    auto kern = cim_bwd_gx_wide_kernel<NB, NB, kWbOBX>;
    CIMQ_TRY(set_lds(kern, p.lds_gx));
    const int slot = prof_begin(KID_BWD_GX, g, s);
    hipLaunchKernelGGL(kern, dim3(g.B * p.v.nbands * p.w.ncc), dim3(256), p.lds_gx, s, g, p.v, p.w, st,
                       reinterpret_cast<const v4i*>(wreg(g, ctx) + L.wcy), pp, sw, sa, gout, x, gx,
                       reinterpret_cast<float*>(ws + W.lsq_part));
    prof_end(slot, s);
    CIMQ_TRY(check_hip("cim_bwd_gx_wide"));
  }
  if (parts & 2) {
    auto kern = cim_bwd_gw_wide_kernel<NB, NB, kWbOBG>;
    CIMQ_TRY(set_lds(kern, p.lds_gw));
    const int slot = prof_begin(KID_BWD_GW, g, s);
    hipLaunchKernelGGL(kern, dim3(p.v.nchunks, p.pairs), dim3(256), p.lds_gw, s, g, p.v, st, ctx + L.xhat, pp, gout,
                       reinterpret_cast<float*>(ws + W.gw_slab), reinterpret_cast<float*>(ws + W.ga_slab));
    prof_end(slot, s);
    CIMQ_TRY(check_hip("cim_bwd_gw_wide"));
  }
  return CIMQ_OK;
}

int launch_wide_bwd(const Geo& g, const PlanWB& p, const uint8_t* ctx, const float* sw, const float* sa,
                    const float* gout, const float* x, float* gx, uint8_t* ws, hipStream_t s, int parts) {
  if (!p.ok || !g.onchw || route_of(g).gx != CIMQ_ROUTE_WIDE_BWD)
    return fail(CIMQ_EINVAL, "internal: the wide backward off its plan");
  if ((parts & 1) && (!x || !gx)) return fail(CIMQ_EINVAL, "internal: the wide grad_x without x / grad_x");
  switch (g.nbw) {
    case 2: return launch_wide_bwd_n<2>(g, p, ctx, sw, sa, gout, x, gx, ws, s, parts);
    case 3: return launch_wide_bwd_n<3>(g, p, ctx, sw, sa, gout, x, gx, ws, s, parts);
    default: return launch_wide_bwd_n<4>(g, p, ctx, sw, sa, gout, x, gx, ws, s, parts);
  }
}

}  // namespace cimq
