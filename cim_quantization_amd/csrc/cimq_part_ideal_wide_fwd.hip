// cimq_part_ideal_wide_fwd.hip -- the large-layer forward of the ideal-ADC conv (cimq_ideal_wide_fwd.hip;
// ideal_wide_fwd_plan in cimq_host.h): cimq_ideal_wide_fwd_abi / _plan and the launcher cimq_ideal_forward dispatches
// to under CIMQ_OPT_WIDE_BWD.  Own translation unit of libcimq.so, compiled without packed fp32 instructions (build.py).
#include "cimq_host.h"
#include "cimq_ideal_wide_fwd.hip"

namespace cimq {

template <int PB>
static int launch_pb(const IdealG& g, const IdealWideFwdG& v, const float* x, const v4i* wf, const float* alpha_a,
                     const float* alpha_w, float* out, hipStream_t s) {
  CIMQ_TRY(set_lds(cim_ideal_fwd_wide_kernel<PB>, g.flds));
  hipLaunchKernelGGL(cim_ideal_fwd_wide_kernel<PB>, dim3((unsigned)(g.B * v.mt), (unsigned)v.ny), dim3(256), g.flds, s,
                     g, v, x, wf, alpha_a, alpha_w, out);
  return check_hip("cim_ideal_fwd_wide");
}

int launch_ideal_wide_fwd(const IdealG& g, const IdealWideFwdG& v, const float* x, const v4i* wf, const float* alpha_a,
                          const float* alpha_w, float* out, hipStream_t s) {
  return v.pb == 4 ? launch_pb<4>(g, v, x, wf, alpha_a, alpha_w, out, s)
                   : launch_pb<2>(g, v, x, wf, alpha_a, alpha_w, out, s);
}

}  // namespace cimq

using namespace cimq;

extern "C" {

int cimq_ideal_wide_fwd_abi(void) { return 1; }

int cimq_ideal_wide_fwd_plan(const cimq_ideal_desc* d, int out[6]) {
  if (!out) return fail(CIMQ_EINVAL, "ideal_wide_fwd_plan: null out");
  for (int i = 0; i < 6; ++i) out[i] = 0;
  if (d && !(d->options & CIMQ_OPT_WIDE_BWD))
    return fail(CIMQ_EUNSUPPORTED, "ideal wide fwd: CIMQ_OPT_WIDE_BWD is not set");
  IdealG g;
  IdealWideG w;
  IdealWideFwdG v;
  int wide = 0;
  CIMQ_TRY(ideal_route(d, &g, &w, &wide));  // (what cimq_ideal_forward plans d with)
  CIMQ_TRY(ideal_wide_fwd_plan(d, g, &v));
  out[0] = 1;
  out[1] = v.mt;
  out[2] = g.nch;
  out[3] = v.gpw;
  out[4] = v.ny;
  out[5] = g.flds;
  return CIMQ_OK;
}

}  // extern "C"
