// cimq_part_ideal_wide.hip -- the large-layer backward pair of the ideal-ADC conv (cimq_ideal_wide.hip; ideal_wide_plan
// in cimq_host.h): cimq_ideal_wide_abi / _plan and the launcher cimq_ideal_backward dispatches to under
// CIMQ_OPT_WIDE_BWD.  Own translation unit of libcimq.so, compiled without packed fp32 instructions (build.py).
#include "cimq_host.h"
#include "cimq_ideal_wide.hip"

namespace cimq {

int launch_ideal_wide_bwd(const IdealG& g, const IdealWideG& v, const float* x, const float* gout, const v4i* wx,
                          const float* alpha_a, const float* alpha_w, float* gx, float* part_a, float* slab,
                          hipStream_t s) {
  CIMQ_TRY(set_lds(cim_ideal_gx_wide_kernel, v.xlds));
  hipLaunchKernelGGL(cim_ideal_gx_wide_kernel, dim3((unsigned)(g.B * v.mt), (unsigned)cdiv(g.ncb, kIdealWideCB)),
                     dim3(256), v.xlds, s, g, v, x, gout, wx, alpha_a, alpha_w, gx, part_a);
  CIMQ_TRY(check_hip("cim_ideal_gx_wide"));
  CIMQ_TRY(set_lds(cim_ideal_gw_wide_kernel, v.wlds));
  hipLaunchKernelGGL(cim_ideal_gw_wide_kernel,
                     dim3((unsigned)g.wslabs, (unsigned)cdiv(g.ncb, 2), (unsigned)cdiv(g.nob, 4)), dim3(256), v.wlds, s,
                     g, v, x, gout, alpha_a, slab);
  return check_hip("cim_ideal_gw_wide");
}

}  // namespace cimq

using namespace cimq;

extern "C" {

int cimq_ideal_wide_abi(void) { return 1; }

int cimq_ideal_wide_plan(const cimq_ideal_desc* d, int out[6]) {
  if (!out) return fail(CIMQ_EINVAL, "ideal_wide_plan: null out");
  for (int i = 0; i < 6; ++i) out[i] = 0;
  IdealG g;
  IdealWideG v;
  CIMQ_TRY(ideal_wide_plan(d, &g, &v));
  out[0] = 1;
  out[1] = v.mt * cdiv(g.ncb, kIdealWideCB);
  out[2] = g.xnoch;
  out[3] = v.wspc;
  out[4] = g.wslabs;
  out[5] = std::max(v.xlds, v.wlds);
  return CIMQ_OK;
}

}  // extern "C"
