// cimq_kernels.hip -- the general forward kernel of the CiM partial-sum-quantised conv (any geometry,
// every ADC variant); the general backward is cimq_kernels_bwd.hip, the prologue kernels cimq_prep.hip.
//
// Data flow (one layer), and where each step lives:
//   prep_act      x (fp32) -> packed per-element act bit-slice codes + int8 ctx code   (cimq_operands.h,
//   prep_weight   w_q      -> int8 MFMA fragments of the weight slices (forward / ps     launched from
//                             recompute), bf16 fragments of the truncated slices (grad_x) cimq_prep.hip)
//   prep_params   alpha_q, sw, sa -> integer ADC thresholds + STE intervals per
//                             (tile, a-slice, w-slice, out-channel)
//   cim_fwd       implicit im2col -> v_mfma_i32_16x16x64_i8 partial sums -> ADC -> shift-add
//   cim_bwd_gx    transposed ps recompute -> STE weights E -> bf16x3 MFMA -> col2im in LDS   (cimq_kernels_bwd.hip)
//   cim_bwd_gw    ps recompute -> STE weights D, ADC codes -> bf16x3 MFMA over pixels -> slabs
//   reduce_*      deterministic slab sums (grad_w, grad_alpha, alpha init), LSQ backward   (cimq_prep.hip)
//
// Every integer step (codes, slices, partial sums, ADC codes, STE masks) is bit-exact with
// the reference's fp32 op sequence; the float reductions are fp32 (bf16x3 on MFMA).
#include "cimq_general.h"

namespace cimq {

// =========================================================================================
// cim_fwd: partial sums + ADC + shift-and-add   (lsq.py:166-233)
// =========================================================================================
// Block = 64 output pixels x one 64-column output-channel group; wave w owns pixels
// [16w, 16w+16).  For every tile i, a-slice j, w-slice k:  ps = X_j(16 x tile) . W_k(tile x 16)
// on v_mfma_i32_16x16x64_i8 (exact integers), then the ADC code and out += code*alpha*mask.
// DBG: additionally write every integer partial sum and its ADC output (before the
// shift-and-add mask) in the reference's [B, T, nbw, nba, P, O] order (the ctx.ps_int of
// lsq.py:192 and adc_out of lsq.py:197-230) -- the parity hook of cimq_debug_partial_sums.
template <int NBP, bool DBG>
__global__ __launch_bounds__(256) void cim_fwd_kernel(Geo g, const int8_t* __restrict__ xcode,
                                                      const v4i* __restrict__ wfrag, Params pp,
                                                      const float* __restrict__ sw_p,
                                                      const float* __restrict__ sa_p,
                                                      float* __restrict__ out, int* __restrict__ ps_dbg,
                                                      float* __restrict__ adc_dbg) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  TileSmem sm;
  sm.As = reinterpret_cast<int8_t*>(smem);
  size_t off = (size_t)g.nba * 64 * g.KTP;
  sm.foff = reinterpret_cast<int*>(smem + off); off += sizeof(int) * g.KS * 64;
  sm.fkk = reinterpret_cast<int*>(smem + off); off += sizeof(int) * g.KS * 64;
  sm.rowinfo = reinterpret_cast<int4*>(smem + off);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, g4 = lane >> 4;
  const int m0 = blockIdx.x * 64;
  const int og = blockIdx.y;
  const int nob = min(4, g.OB16 - og * 4);
  const float sw = *sw_p, sa = *sa_p;
  const bool literal = (pp.flags[0] != 0) || g.mode != ADC_TERNARY || g.variant != VAR_LIBRARY;
  const int nkj = g.nbw * g.nba;

  build_rowinfo(g, m0, sm.rowinfo);
  float acc_out[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc_out[a][b] = 0.f;

  for (int i = 0; i < g.T; ++i) {
    __syncthreads();
    build_ftable(g, i, sm.foff, sm.fkk);
    __syncthreads();
    build_As<NBP>(g, xcode, sm);
    __syncthreads();
    for (int j = 0; j < g.nba; ++j) {
      v4i a[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        if (ks < g.KS) a[ks] = load_xfrag(g, sm.As, j, wave * 16 + r16, ks, lane);
      for (int k = 0; k < g.nbw; ++k) {
        const float mk = pp.ckj[k * g.nba + j];
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) {
          if (ob < nob) {
            const int nb = k * g.OB16 + og * 4 + ob;
            v4i acc = {0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
              if (ks < g.KS)
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(
                    a[ks], wfrag[((size_t)(i * g.KS + ks) * g.NBLK + nb) * WAVE + lane], acc, 0, 0, 0);
            const int o = (og * 4 + ob) * 16 + r16;
            const int pi = pidx(g, i, j, k, o);
            if (DBG) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int m = m0 + wave * 16 + 4 * g4 + r;
                if (m < g.M && o < g.O) {
                  const int b = m / g.P, p = m - b * g.P;
                  const size_t di = ((((size_t)b * g.T + i) * g.nbw + k) * g.nba + j) * g.P * g.O +
                                    (size_t)p * g.O + o;
                  ps_dbg[di] = acc[r];
                  float adc;
                  if (!literal) {
                    const float q = (acc[r] >= pp.thi[pi]) ? 1.f : ((acc[r] <= pp.tlo[pi]) ? -1.f : 0.f);
                    adc = q * pp.alpha[pi];
                  } else {
                    adc = adc_value(g, acc[r], sw, sa, pp.alpha[pi], pp.beta[pi], (uint64_t)di);
                  }
                  adc_dbg[di] = adc;
                }
              }
            }
            if (!literal) {
              const int thi = pp.thi[pi], tlo = pp.tlo[pi];
              const float cf = pp.coef[pi];
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int ps = acc[r];
                float v = (ps >= thi) ? cf : 0.f;
                v -= (ps <= tlo) ? cf : 0.f;
                acc_out[ob][r] += v;
              }
            } else {
              const float al = pp.alpha[pi], be = pp.beta[pi];
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                uint64_t eid = 0;  // element id of the stochastic ADC's draws: [B, T, nbw, nba, P, O] order
                if (g.variant == VAR_STOCHASTIC) {
                  const int m = m0 + wave * 16 + 4 * g4 + r;
                  const int b = m / g.P, p = m - b * g.P;
                  eid = ((((uint64_t)b * g.T + i) * g.nbw + k) * g.nba + j) * (uint64_t)g.P * g.O + (uint64_t)p * g.O + o;
                }
                const float adc = adc_value(g, acc[r], sw, sa, al, be, eid);
                acc_out[ob][r] += adc * mk;
              }
            }
          }
        }
      }
    }
  }
  (void)nkj;
#pragma unroll
  for (int ob = 0; ob < 4; ++ob) {
    if (ob < nob) {
      const int o = (og * 4 + ob) * 16 + r16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wave * 16 + 4 * g4 + r;
        if (m < g.M && o < g.O) out[(size_t)m * g.O + o] = acc_out[ob][r];
      }
    }
  }
}

}  // namespace cimq
