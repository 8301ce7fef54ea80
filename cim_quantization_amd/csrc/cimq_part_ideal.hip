// cimq_part_ideal.hip -- entry points and launches of the ideal-ADC conv (cimq_ideal.hip; ideal_plan in
// cimq_host.h): cimq_ideal_abi / _plan / _sizes / _forward / _backward.  Own translation unit of libcimq.so, compiled
// without packed fp32 instructions (build.py).
#include "cimq_host.h"
#include "cimq_ideal.hip"

using namespace cimq;

namespace {

int gw_tail_blocks(const IdealG& g) {
  return (int)std::max(1LL, std::min<long long>(((long long)g.O * g.C * g.ntap + 255) / 256, kIdealTailBlocks));
}

// what a descriptor runs on: ideal_plan's kernels, or under CIMQ_OPT_WIDE_BWD where ideal_wide_plan holds the wide
// backward pair (cimq_part_ideal_wide.hip); the forward of either is cim_ideal_fwd_kernel, or under the same hint where
// ideal_wide_fwd_plan holds the large-layer forward (cimq_part_ideal_wide_fwd.hip) on the same plan and fragments
struct IdealRoute {
  IdealG g;
  IdealWideG v;
  int wide;
  int gx_blocks() const { return wide ? v.gxblocks : ideal_gx_blocks(g); }
};
int route(const cimq_ideal_desc* d, IdealRoute* r) { return ideal_route(d, &r->g, &r->v, &r->wide); }

// ws: act-LSQ partials | weight-LSQ partials | grad_w slabs
struct IdealWs {
  size_t part_a, part_w, slab, total;
};
IdealWs ideal_ws(const IdealG& g, int gx_blocks) {
  IdealWs w;
  w.part_a = 0;
  w.part_w = align256((size_t)gx_blocks * 4);
  w.slab = w.part_w + align256((size_t)kIdealTailBlocks * 4);
  w.total = w.slab + align256((size_t)g.wslabs * g.OP * g.ntap * g.Cp * 4);
  return w;
}

template <int NOB>
int launch_fwd(const IdealG& g, const float* x, const v4i* wf, const float* aa, const float* aw, float* out,
               hipStream_t st) {
  const dim3 grid((unsigned)(g.B * g.mt), (unsigned)cdiv(g.nob, NOB));
  if (g.split) {
    CIMQ_TRY(set_lds(cim_ideal_fwd_kernel<NOB, true>, g.flds));
    hipLaunchKernelGGL((cim_ideal_fwd_kernel<NOB, true>), grid, dim3(256), g.flds, st, g, x, wf, aa, aw, out);
  } else {
    CIMQ_TRY(set_lds(cim_ideal_fwd_kernel<NOB, false>, g.flds));
    hipLaunchKernelGGL((cim_ideal_fwd_kernel<NOB, false>), grid, dim3(256), g.flds, st, g, x, wf, aa, aw, out);
  }
  return check_hip("cim_ideal_fwd");
}

}  // namespace

extern "C" {

int cimq_ideal_abi(void) { return 1; }

int cimq_ideal_plan(const cimq_ideal_desc* d, int out[5]) {
  if (!out) return fail(CIMQ_EINVAL, "ideal_plan: null out");
  for (int i = 0; i < 5; ++i) out[i] = 0;
  IdealRoute r;
  CIMQ_TRY(route(d, &r));
  const IdealG& g = r.g;
  out[0] = 1;
  out[1] = g.mt;
  out[2] = g.nch;
  out[3] = g.xnrb * g.xncol;
  out[4] = g.wslabs;
  return CIMQ_OK;
}

int cimq_ideal_sizes(const cimq_ideal_desc* d, size_t* ctx_bytes, size_t* ws_bytes) {
  IdealRoute r;
  CIMQ_TRY(route(d, &r));
  const IdealG& g = r.g;
  if (ctx_bytes) *ctx_bytes = ideal_wf_bytes(g) + (g.inference ? 0 : ideal_wx_bytes(g));
  if (ws_bytes) *ws_bytes = ideal_ws(g, r.gx_blocks()).total;
  return CIMQ_OK;
}

int cimq_ideal_forward(const cimq_ideal_desc* d, const float* x, const float* weight, const float* alpha_act,
                       const float* alpha_weight, float* out, void* ctx, void* ws, void* stream) {
  (void)ws;
  IdealRoute r;
  CIMQ_TRY(route(d, &r));
  const IdealG& g = r.g;
  if (!x || !weight || !alpha_act || !alpha_weight || !out || !ctx)
    return fail(CIMQ_EINVAL, "ideal_forward: null pointer");
  hipStream_t st = (hipStream_t)stream;
  v4i* wf = reinterpret_cast<v4i*>(ctx);
  v4i* wx = reinterpret_cast<v4i*>(reinterpret_cast<uint8_t*>(ctx) + ideal_wf_bytes(g));
  const long long nfrag = (long long)g.nch * g.fks * g.nob * 64 + (g.inference ? 0 : (long long)g.ncb * g.xnoch * g.xks * 64);
  hipLaunchKernelGGL(ideal_prep_w_kernel, dim3((unsigned)std::min<long long>((nfrag + 255) / 256, 4096)), dim3(256), 0,
                     st, g, weight, alpha_weight, wf, wx);
  CIMQ_TRY(check_hip("ideal_prep_w"));
  // the hint, in training and in inference descriptors alike: the large-layer forward where its plan holds
  IdealWideFwdG fv;
  if ((d->options & CIMQ_OPT_WIDE_BWD) && ideal_wide_fwd_plan(d, g, &fv) == CIMQ_OK)
    return launch_ideal_wide_fwd(g, fv, x, wf, alpha_act, alpha_weight, out, st);
  if (g.nobw == 4) return launch_fwd<4>(g, x, wf, alpha_act, alpha_weight, out, st);
  if (g.nobw == 2) return launch_fwd<2>(g, x, wf, alpha_act, alpha_weight, out, st);
  return launch_fwd<1>(g, x, wf, alpha_act, alpha_weight, out, st);
}

int cimq_ideal_backward(const cimq_ideal_desc* d, const float* x, const float* weight, const float* alpha_act,
                        const float* alpha_weight, const float* grad_out, const void* ctx, float* grad_x,
                        float* grad_w, float* grad_alpha_act, float* grad_alpha_weight, void* ws, void* stream) {
  IdealRoute r;
  CIMQ_TRY(route(d, &r));
  const IdealG& g = r.g;
  if (g.inference) return fail(CIMQ_EINVAL, "ideal_backward: an inference descriptor has no backward");
  if (!x || !weight || !alpha_act || !alpha_weight || !grad_out || !ctx || !grad_x || !grad_w || !grad_alpha_act ||
      !grad_alpha_weight || !ws)
    return fail(CIMQ_EINVAL, "ideal_backward: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const IdealWs W = ideal_ws(g, r.gx_blocks());
  uint8_t* wsb = reinterpret_cast<uint8_t*>(ws);
  float* part_a = reinterpret_cast<float*>(wsb + W.part_a);
  float* part_w = reinterpret_cast<float*>(wsb + W.part_w);
  float* slab = reinterpret_cast<float*>(wsb + W.slab);
  const v4i* wx = reinterpret_cast<const v4i*>(reinterpret_cast<const uint8_t*>(ctx) + ideal_wf_bytes(g));

  if (r.wide) {
    CIMQ_TRY(launch_ideal_wide_bwd(g, r.v, x, grad_out, wx, alpha_act, alpha_weight, grad_x, part_a, slab, st));
  } else {
    CIMQ_TRY(set_lds(cim_ideal_gx_kernel, g.xlds));
    hipLaunchKernelGGL(cim_ideal_gx_kernel, dim3((unsigned)(g.B * g.xnrb * g.xncol), (unsigned)cdiv(g.ncb, kIdealCBX)),
                       dim3(256), g.xlds, st, g, x, grad_out, wx, alpha_act, alpha_weight, grad_x, part_a);
    CIMQ_TRY(check_hip("cim_ideal_gx"));

    CIMQ_TRY(set_lds(cim_ideal_gw_kernel, g.wlds));
    hipLaunchKernelGGL(cim_ideal_gw_kernel,
                       dim3((unsigned)g.wslabs, (unsigned)(g.ncb * g.wntg), (unsigned)cdiv(g.nob, kIdealOBG)),
                       dim3(256), g.wlds, st, g, x, grad_out, alpha_act, slab);
    CIMQ_TRY(check_hip("cim_ideal_gw"));
  }

  const int ntb = gw_tail_blocks(g);
  hipLaunchKernelGGL(ideal_gw_finish_kernel, dim3(ntb), dim3(256), 0, st, g, weight, slab, alpha_act, alpha_weight,
                     grad_w, part_w);
  CIMQ_TRY(check_hip("ideal_gw_finish"));
  hipLaunchKernelGGL(ideal_alpha_finish_kernel, dim3(1), dim3(256), 0, st, g, r.gx_blocks(), part_a, ntb, part_w,
                     grad_alpha_act, grad_alpha_weight);
  return check_hip("ideal_alpha_finish");
}

}  // extern "C"
