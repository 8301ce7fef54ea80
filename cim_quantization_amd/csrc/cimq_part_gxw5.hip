// cimq_part_gxw5.hip -- launches of the w3a3 stride-1 16 / 32-channel layers' backward: the per-input-pixel grad_x
// kernel (cimq_gx5.hip, lsq.py:336-386 + lsq.py:549), the grad_w / grad_alpha kernel (cimq_gw5.hip,
// lsq.py:321-356), and both in ONE launch: the workgroups of cim_bwd_gx5_kernel first, then those of
// cim_bwd_gw5_kernel, each running its own body.  The two kernels read the same state words and grad_out and are
// independent; as one grid, grad_w's workgroups start on the CUs grad_x's last workgroups leave idle, and the
// launch gap between them goes.  Own translation unit of libcimq.so.
#include "cimq_host.h"
#include "cimq_gx5.hip"
#include "cimq_gw5.hip"

namespace cimq {

int launch_gx5(const Geo& g, const PlanX5& p, const uint8_t* ctx, const float* sw, const float* sa, const float* gout,
               const float* x, float* gx, uint8_t* ws, hipStream_t s) {
  if (!p.ok) return fail(CIMQ_EINVAL, "internal: cim_bwd_gx5 off its plan");
  CtxLayout L = ctx_layout(g);
  WsLayout W = ws_layout(g);
  auto kern = p.v.CBN == 2 ? cim_bwd_gx5_kernel<2> : cim_bwd_gx5_kernel<1>;
  CIMQ_TRY(set_lds(kern, p.lds));
  const int slot = prof_begin(KID_GX_V8, g, s);
  hipLaunchKernelGGL(kern, dim3(p.nblk), dim3(512), p.lds, s, g, p.v, reinterpret_cast<const uint32_t*>(ctx + L.st),
                     reinterpret_cast<const v4i*>(wreg(g, ctx) + L.wg5), params_of(g, const_cast<uint8_t*>(ctx)), sw,
                     sa, gout, x, gx, reinterpret_cast<float*>(ws + W.lsq_part));
  prof_end(slot, s);
  return check_hip("cim_bwd_gx5");
}

int launch_prep_wg5(const Geo& g, const float* w_q, const float* sw, uint8_t* ctx, hipStream_t s) {
  const int total = (int)(x5_frag_bytes(g) / 16);
  if (total == 0) return CIMQ_OK;
  CtxLayout L = ctx_layout(g);
  hipLaunchKernelGGL(prep_wg5_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, g, w_q, sw, total,
                     reinterpret_cast<v4i*>(wreg(g, ctx) + L.wg5));
  return check_hip("prep_wg5");
}

int launch_gw5(const Geo& g, const PlanG5& p, const uint8_t* ctx, const float* gout, uint8_t* ws, hipStream_t s) {
  if (!p.ok) return fail(CIMQ_EINVAL, "internal: cim_bwd_gw5 off its plan");
  CtxLayout L = ctx_layout(g);
  WsLayout W = ws_layout(g);
  if (W.nchunks_bwd != p.v.nchunks) return fail(CIMQ_EINVAL, "internal: cim_bwd_gw5 slab count mismatch");
  G5 v = p.v;
  v.codes = route_of(g).codes ? 1 : 0;  // the forward wrote code bytes (cim_fwd5_kernel on the module path)
  // the row-block split compiled in: 16 input channels (every block in input-channel block 0) and 32 (blocks 0 / 1)
  const int sp = !tune("GW5_SP8", 1) ? 0 : g.C == 16 ? 8 : (g.C == 32 && tune("GW5_SP78", 1)) ? 78 : 0;
#define CIMQ_GW5_K(SS_, C_) (sp == 8 ? cim_bwd_gw5_kernel<SS_, C_, 8> : sp == 78 ? cim_bwd_gw5_kernel<SS_, C_, 78> \
                                                                       : cim_bwd_gw5_kernel<SS_, C_, 0>)
  auto kern = g.SH == 2 ? (v.codes ? CIMQ_GW5_K(2, true) : CIMQ_GW5_K(2, false))
                        : (v.codes ? CIMQ_GW5_K(1, true) : CIMQ_GW5_K(1, false));
#undef CIMQ_GW5_K
  CIMQ_TRY(set_lds(kern, p.lds));
  const int slot = prof_begin(KID_GW_V7, g, s);
  hipLaunchKernelGGL(kern, dim3(p.v.nchunks, p.pairs), dim3(512), p.lds, s, g, v,
                     reinterpret_cast<const uint32_t*>(ctx + L.st), reinterpret_cast<const uint32_t*>(ctx + L.xhat),
                     params_of(g, const_cast<uint8_t*>(ctx)), gout, reinterpret_cast<const uint32_t*>(ctx + L.alut),
                     reinterpret_cast<float*>(ws + W.gw_slab), reinterpret_cast<float*>(ws + W.ga_slab));
  prof_end(slot, s);
  return check_hip("cim_bwd_gw5");
}

template <int CBN, bool CODES, int SP>
__global__ __attribute__((amdgpu_flat_work_group_size(512, 512), amdgpu_waves_per_eu(4, 4)))
void cim_bwd_gxw5_kernel(Geo g, X5 vx, G5 vw, const uint32_t* __restrict__ st, const v4i* __restrict__ wg5, Params pp,
                         const float* __restrict__ sw_p, const float* __restrict__ sa_p, const float* __restrict__ gout,
                         const float* __restrict__ x, float* __restrict__ gx, float* __restrict__ gsa_part,
                         const uint32_t* __restrict__ xcb, const uint32_t* __restrict__ cal, float* __restrict__ gw_slab,
                         float* __restrict__ ga_slab, int ngx) {
  const int b = (int)blockIdx.x;
  if (b < ngx) {
    gx5_body<CBN>(b, ngx, g, vx, st, wg5, pp, sw_p, sa_p, gout, x, gx, gsa_part);
  } else {
    const int t = b - ngx, by = t / vw.nchunks;
    gw5_body<1, CODES, SP>(t - by * vw.nchunks, by, g, vw, st, xcb, pp, gout, cal, gw_slab, ga_slab);
  }
}

int launch_gxw5(const Geo& g, const PlanX5& px, const PlanG5& pw, const uint8_t* ctx, const float* sw, const float* sa,
                const float* gout, const float* x, float* gx, uint8_t* ws, hipStream_t s) {
  if (!px.ok || !pw.ok || g.SH != 1 || !(g.C == 16 || g.C == 32)) return fail(CIMQ_EINVAL, "internal: cim_bwd_gxw5 off its plans");
  CtxLayout L = ctx_layout(g);
  WsLayout W = ws_layout(g);
  if (W.nchunks_bwd != pw.v.nchunks) return fail(CIMQ_EINVAL, "internal: cim_bwd_gxw5 slab count mismatch");
  G5 vw = pw.v;
  vw.codes = route_of(g).codes ? 1 : 0;  // the forward wrote code bytes (cim_fwd5_kernel on the module path)
  // x5_plan: C = 16 -> one 16-channel input block (gw5's row-block split at 8), C = 32 -> two (splits 8 and 7)
  auto kern = px.v.CBN == 1 ? (vw.codes ? cim_bwd_gxw5_kernel<1, true, 8> : cim_bwd_gxw5_kernel<1, false, 8>)
                            : (vw.codes ? cim_bwd_gxw5_kernel<2, true, 78> : cim_bwd_gxw5_kernel<2, false, 78>);
  const size_t lds = std::max(px.lds, pw.lds);
  CIMQ_TRY(set_lds(kern, lds));
  const int ngw = pw.v.nchunks * pw.pairs;
  // timed as the fused family (grad_x + grad_w of the layer in one launch: its algorithmic bytes are read gy
  // and x once, write gx; its MFMA work both contractions), not as grad_x alone
  const int slot = prof_begin(KID_FUSED, g, s);
  hipLaunchKernelGGL(kern, dim3(px.nblk + ngw), dim3(512), lds, s, g, px.v, vw, reinterpret_cast<const uint32_t*>(ctx + L.st),
                     reinterpret_cast<const v4i*>(wreg(g, ctx) + L.wg5), params_of(g, const_cast<uint8_t*>(ctx)), sw, sa,
                     gout, x, gx, reinterpret_cast<float*>(ws + W.lsq_part), reinterpret_cast<const uint32_t*>(ctx + L.xhat),
                     reinterpret_cast<const uint32_t*>(ctx + L.alut), reinterpret_cast<float*>(ws + W.gw_slab),
                     reinterpret_cast<float*>(ws + W.ga_slab), px.nblk);
  prof_end(slot, s);
  return check_hip("cim_bwd_gxw5");
}

}  // namespace cimq
