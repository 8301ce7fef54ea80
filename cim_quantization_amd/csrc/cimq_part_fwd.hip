// cimq_part_fwd.hip -- forward launch sequences (lsq.py:166-233): the v3 fast-path kernel and
// the general kernel (also the partial-sum debug hook).  Own translation unit of libcimq.so.
#include "cimq_host.h"
#include "cimq_kernels.hip"
#include "cimq_kernels_v3.hip"

namespace cimq {

using Fwd3Kern = void (*)(Geo, V3, const uint8_t*, const v4i*, Params, const float*, const float*, float*, uint8_t*,
                          const float*, const float*, uint8_t*, Epi);

// the OBM 1 / 2 / 4 instances of one (format, state, mode), up to the widest one built
template <int NBP, int KS, int CST, FwdState ST, FwdMode M, int OBMAX>
Fwd3Kern fwd3_obm(int obm) {
  if constexpr (OBMAX == 1) return cim_fwd_v3_kernel<NBP, KS, CST, ST, M, 1>;
  else if constexpr (OBMAX == 2) return obm == 1 ? cim_fwd_v3_kernel<NBP, KS, CST, ST, M, 1> : cim_fwd_v3_kernel<NBP, KS, CST, ST, M, 2>;
  else return obm == 1 ? cim_fwd_v3_kernel<NBP, KS, CST, ST, M, 1> : obm == 2 ? cim_fwd_v3_kernel<NBP, KS, CST, ST, M, 2>
                                                                            : cim_fwd_v3_kernel<NBP, KS, CST, ST, M, 4>;
}

// cim_fwd_v3_kernel's instance of one mode for (format, state, OBM).  The compact formats' state in a mode is S: the
// epilogue and later modes are forward only.  The first conv's training instance writes no state either, so every
// forward-only call without an epilogue runs it as it is (named here, where the code object has always had it;
// CST 0's, for the same reason, in launch_fwd_v3).  w2a2 with an epilogue: two blocks at the most (launch_fwd_v3)
template <int NBP, int KS, FwdMode M>
Fwd3Kern fwd3_kernel(int cst, FwdState st, int obm) {
  constexpr FwdState S = M == FwdMode::TRAIN ? FwdState::WRITE : FwdState::NONE;
  if constexpr (M != FwdMode::INFER)
    if (cst == 0) return fwd3_obm<NBP, KS, 0, FwdState::WRITE, M, 4>(obm);
  if constexpr (NBP == 8)  // v7_plan: w8a8 with one 16-channel block
    return st == FwdState::RECOMPUTE ? fwd3_obm<8, KS, 8, FwdState::RECOMPUTE, M == FwdMode::INFER ? FwdMode::TRAIN : M, 1>(obm)
                                     : fwd3_obm<8, KS, 8, S, M, 1>(obm);
  else if (cst != 4)
    return cst == 2 ? fwd3_obm<NBP, KS, 2, S, M, has_epi(M) ? 2 : 4>(obm) : fwd3_obm<NBP, KS, 3, S, M, 4>(obm);
  // w4a4 word pairs: the training forward writes them (v7_w44), every forward-only mode runs their stateless form
  // (v7_w44_eval); two blocks at the most (named last, the stateless ones after the training one: the older
  // instances keep their places in the code object)
  if constexpr (NBP == 4 && M == FwdMode::TRAIN) return fwd3_obm<4, KS, 4, FwdState::WRITE, FwdMode::TRAIN, 2>(obm);
  else if constexpr (NBP == 4) return st == FwdState::NONE ? fwd3_obm<4, KS, 4, FwdState::NONE, M, 2>(obm) : nullptr;
  return nullptr;
}

template <int NBP, int KS>
int launch_fwd_v3(const Geo& g, const Plan3& p, uint8_t* ctx, const float* sw, const float* sa, float* out,
                  hipStream_t s, const ActQ* aq, const Epi* ep = nullptr, bool q8 = false) {
  CtxLayout L = ctx_layout(g);
  // CST, fixed at compile time: 0 per-k state words (the general backward's), else the compact ones the v7-plan
  // backwards read -- nbw = nba = CST (2, 3, 4), 8 the w8a8 planes.  The first conv's backward recomputes them; a
  // forward-only call (CIMQ_OPT_INFERENCE) runs the same instances without the state words, their bits and the
  // backward words (CST 0 and the first conv's write no state as they are)
  const int cst = route_of(g).cst;
  const FwdState st = route_of(g).fst;
  FwdMode m = fwd_mode_of(g, ep);
  if (has_epi(m) && (!g.inference || !g.onchw))
    return fail(CIMQ_EINVAL, "internal: output epilogue off the forward-only module path");
  if (m == FwdMode::INFER && cst == 0) m = FwdMode::TRAIN;
  // OBM: 16-channel output blocks per block (register arrays sized for exactly that)
  int obm = std::min(p.v.obm, g.OB16 <= 2 ? g.OB16 : 4);
  // (the w2a2 four-block instances sit at a VGPR step -- 127 and 160 -- and the epilogue's residual float4 would
  // cost them a wave per SIMD: with an epilogue those layers run the two-block instances, twice the blocks in y;
  // the plan's LDS figures, made for four blocks, cover two)
  if (has_epi(m) && cst == 2 && st == FwdState::NONE && obm == 4) obm = 2;
  // (w4a4 word pairs: 16 slice pairs per output block -- instances of one and two blocks; the words are the
  // training forward's, a forward-only mode runs the stateless form)
  if (cst == 4) {
    if ((m == FwdMode::TRAIN) != (st == FwdState::WRITE) || (m != FwdMode::TRAIN && st != FwdState::NONE))
      return fail(CIMQ_EINVAL, "internal: the w4a4 state words outside a training forward");
    if (obm == 4) obm = 2;
  }
  // (the modes in the order the code object has always had its instances: a kernel's place decides its addresses)
  Fwd3Kern kern = nullptr;
  switch (m) {
    case FwdMode::CODES: kern = fwd3_kernel<NBP, KS, FwdMode::CODES>(cst, st, obm); break;
    case FwdMode::EPI: kern = fwd3_kernel<NBP, KS, FwdMode::EPI>(cst, st, obm); break;
    case FwdMode::INFER: kern = fwd3_kernel<NBP, KS, FwdMode::INFER>(cst, st, obm); break;
    case FwdMode::TRAIN: kern = fwd3_kernel<NBP, KS, FwdMode::TRAIN>(cst, st, obm); break;
    case FwdMode::VIEW: kern = fwd3_kernel<NBP, KS, FwdMode::VIEW>(cst, st, obm); break;
  }
  // q8 (launch_fwd8_staged): the w8a8 epilogue instance whose row staging quantises aq->x itself
  if (q8) {
    kern = nullptr;
    if constexpr (NBP == 8) {
      if (m == FwdMode::EPI && cst == 8 && aq)  // one 16-channel block (the ResNets' first conv)
        kern = st == FwdState::RECOMPUTE ? cim_fwd_v3_kernel<8, KS, 8, FwdState::RECOMPUTE, FwdMode::EPI, 1, true>
                                         : cim_fwd_v3_kernel<8, KS, 8, FwdState::NONE, FwdMode::EPI, 1, true>;
      if (m == FwdMode::EPI && cst == 0 && aq)  // wider (VGG's 3 -> 128): the per-k form, as fwd3_kernel names it
        kern = obm == 1   ? cim_fwd_v3_kernel<8, KS, 0, FwdState::WRITE, FwdMode::EPI, 1, true>
               : obm == 2 ? cim_fwd_v3_kernel<8, KS, 0, FwdState::WRITE, FwdMode::EPI, 2, true>
                          : cim_fwd_v3_kernel<8, KS, 0, FwdState::WRITE, FwdMode::EPI, 4, true>;
    }
    if (!kern) return fail(CIMQ_EINVAL, "internal: the staged w8a8 quantiser off its plan");
  }
  // the fused activation quantiser's word table (after the kernel's other LDS)
  const size_t lds = p.lds_fwd + (aq ? (size_t)kActLutMax * 2 * 4 : 0);
  CIMQ_TRY(set_lds(kern, lds));
  // grid: about three resident 256-thread blocks per CU (measured: 768 blocks for w3a3, 1024
  // for the 236-VGPR w8a8 instance)
  dim3 grid(std::min(p.v.nmt, tune("FWD_GRID", NBP == 8 ? 1024 : 768)), cdiv(g.OB16, obm));
  const int slot = prof_begin(cst ? KID_FWD_V7 : KID_FWD, g, s);
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, g, p.v, ctx + L.xcode,
                     reinterpret_cast<const v4i*>(wreg(g, ctx) + L.wfrag), params_of(g, ctx), sw, sa, out, ctx + L.st,
                     aq ? aq->x : nullptr, aq ? aq->signed_act : nullptr, aq ? ctx + L.xhat : nullptr,
                     ep ? *ep : Epi{});
  prof_end(slot, s);
  return check_hip("cim_fwd_v3");
}

template <int NBP, bool DBG>
int launch_fwd(const Geo& g, uint8_t* ctx, const float* sw, const float* sa, float* out, int* ps_dbg,
               float* adc_dbg, hipStream_t s, const ActQ* aq, const Epi* ep = nullptr) {
  CtxLayout L = ctx_layout(g);
  const Plan3 p = v3_plan(g);
  if (p.ok && !DBG) {
    // (cim_fwd5_kernel writes NCHW only: a forward-only Function call, [B, P, O], stays on cim_fwd_v3_kernel)
    if (aq && route_of(g).fwd == CIMQ_ROUTE_FWD5) return launch_fwd5(g, f5_plan(g), ctx, sw, sa, out, s, aq, ep);
    if (g.KS == 1) return launch_fwd_v3<NBP, 1>(g, p, ctx, sw, sa, out, s, aq, ep);
    return launch_fwd_v3<NBP, 2>(g, p, ctx, sw, sa, out, s, aq, ep);
  }
  // (the general kernel writes [B, P, O]: the module's epilogue is bpo_to_nchw_epi_kernel's)
  if (ep) return fail(CIMQ_EINVAL, "internal: output epilogue on the general forward kernel");
  if (p.ok) {
    // the debug forward is the general kernel; the fast one still fills the state words the
    // fast backward reads (same out values)
    if (g.KS == 1) CIMQ_TRY((launch_fwd_v3<NBP, 1>(g, p, ctx, sw, sa, out, s, nullptr)));
    else CIMQ_TRY((launch_fwd_v3<NBP, 2>(g, p, ctx, sw, sa, out, s, nullptr)));
  }
  dim3 grid(cdiv(g.M, 64), cdiv(g.OB16, 4));
  const size_t lds = lds_tile(g);
  auto kern = cim_fwd_kernel<NBP, DBG>;
  CIMQ_TRY(set_lds(kern, lds));
  const int slot = DBG ? -1 : prof_begin(KID_FWD, g, s);
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, g, reinterpret_cast<const int8_t*>(ctx + L.xcode),
                     reinterpret_cast<const v4i*>(wreg(g, ctx) + L.wfrag), params_of(g, ctx), sw, sa, out, ps_dbg,
                     adc_dbg);
  prof_end(slot, s);
  return check_hip("cim_fwd");
}


int launch_fwd8_staged(const Geo& g, uint8_t* ctx, const float* sw, const float* sa, float* out, hipStream_t s,
                       const ActQ* aq, const Epi* ep) {
  if (!fwd8_stage_ok(g) || !aq || !ep) return fail(CIMQ_EINVAL, "internal: the staged w8a8 quantiser off its plan");
  const Plan3 p = v3_plan(g);
  if (g.KS == 1) return launch_fwd_v3<8, 1>(g, p, ctx, sw, sa, out, s, aq, ep, true);
  return launch_fwd_v3<8, 2>(g, p, ctx, sw, sa, out, s, aq, ep, true);
}

int launch_fwd_any(const Geo& g, uint8_t* ctx, const float* sw, const float* sa, float* out, int* ps_dbg,
                   float* adc_dbg, hipStream_t s, const ActQ* aq, const Epi* ep) {
  const Route r = route_of(g);
  if (aq && (!r.actq || ps_dbg)) return fail(CIMQ_EINVAL, "internal: fused activation quantiser off its plan");
  if (ep && (ps_dbg || !g.inference)) return fail(CIMQ_EINVAL, "internal: output epilogue off the forward-only path");
  if (r.fwd == CIMQ_ROUTE_WIDE) {
    if (ps_dbg) return fail(CIMQ_EINVAL, "internal: the debug hook on the wide forward");
    return launch_wide(g, wide_plan(g), ctx, sw, sa, out, s, aq, ep);
  }
  if (r.fwd == CIMQ_ROUTE_DENSE) {
    // the dense GEMM path (its state words feed the dense backward); the debug hook then reruns
    // the general kernel for the partial sums (same out values)
    CIMQ_TRY(launch_dense_fwd(g, ctx, sw, sa, out, s, ep));
    if (!ps_dbg) return CIMQ_OK;
  }
  if (ps_dbg) {
    if (g.NBP == 4) return launch_fwd<4, true>(g, ctx, sw, sa, out, ps_dbg, adc_dbg, s, nullptr);
    return launch_fwd<8, true>(g, ctx, sw, sa, out, ps_dbg, adc_dbg, s, nullptr);
  }
  if (g.NBP == 4) return launch_fwd<4, false>(g, ctx, sw, sa, out, nullptr, nullptr, s, aq, ep);
  return launch_fwd<8, false>(g, ctx, sw, sa, out, nullptr, nullptr, s, nullptr, ep);
}

}  // namespace cimq
