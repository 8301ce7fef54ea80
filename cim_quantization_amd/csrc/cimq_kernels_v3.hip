// cimq_kernels_v3.hip -- fast path for layers whose output image splits into whole-row
// 64-pixel tiles (P % 64 == 0 and Wo | 64: every conv of the CIFAR ResNets).  Same
// arithmetic as the general kernels in cimq_kernels.hip (bit-exact integer partial sums, ADC
// codes and STE masks; fp32-accurate bf16x3 backward GEMMs); the data movement is built for
// CDNA4:
//   * the packed activation slice words of a pixel strip (or, for grad_x, of a band of input
//     rows) are staged into LDS once with batched 16-byte loads, zero-padded like nn.Unfold;
//   * each wave gathers the int8 MFMA operand of ITS 16 pixels straight from that patch
//     (16 LDS words per 64-deep K-step, v_perm byte transposes give every bit slice at once),
//     so there is no im2col buffer, no LDS round trip and no barrier between the waves;
//   * per-tile weight fragments, ADC thresholds and STE intervals live in LDS; every index
//     into them is a table lookup or a shift (no integer division in the inner loops);
//   * grad_x blocks own a band of input rows and fold (nn.Fold adjoint) into an LDS
//     accumulator with the same geometry as the patch -- the fold address of (pixel, f) is
//     the gather address -- then apply the fused LSQ activation backward and store once;
//   * grad_w keeps its accumulators in registers across the block's pixel chunk and folds the
//     four waves together in LDS once, at the end.
#include "cimq_fwd_stage.h"

namespace cimq {

// ---------------------------------------------------------------------------------------
// forward: out[m, o] = sum_{i,j,k} ADC(ps_ijk[m, o]) * mask   (lsq.py:166-233)
// block = 64-pixel m-tiles (grid-stride) x one 64-wide o-group; wave w = pixels 16w..16w+15.
// ---------------------------------------------------------------------------------------

// The kernel's repeated pieces, one definition each: free functions with scalars by value, the form that keeps every
// instance's instruction stream.  The weight side's items, global -> LDS, first: the stagings
// (stage_tile, stage_prm, stage_all, load_tile) differ only in the tile index they pass.  Item idx of tile i's
// weight fragments [k][ob][ks][64] (zero past the o-group's last output block):
template <int KS, int OBM>
__device__ inline v4i frag_item(const Geo& g, const v4i* __restrict__ wf, int og, int nob, int lnob, int i, int idx) {
  const int l = idx & 63, fr = idx >> 6;
  const int ks = KS == 1 ? 0 : (fr & 1), kob = KS == 1 ? fr : (fr >> 1);
  const int k = kob >> lnob, ob = kob - (k << lnob);
  v4i w = {0, 0, 0, 0};
  if (ob < nob) w = wf[((size_t)(i * KS + ks) * g.NBLK + k * g.OB16 + og * OBM + ob) * WAVE + l];
  return w;
}
// item idx of tile i's ADC thresholds / STE intervals [j][k][NOB*16] (NOB = 1 << lnob), and of its coefficients
template <int OBM>
__device__ inline int4 thr_item(const Geo& g, const Params& pp, int og, int lnob, float inv_nbw, int i, int idx) {
  const int col = idx & ((16 << lnob) - 1), jk = idx >> (4 + lnob);
  const int j = fdiv(jk, g.nbw, inv_nbw), k = jk - j * g.nbw;
  const int o = og * OBM * 16 + col;
  int4 p = make_int4(0, 0, 0, 0);
  if (o < g.Opad) {
    const int pi = pidx(g, i, j, k, o);
    p = make_int4(pp.thi[pi], pp.tlo[pi], pp.mlo[pi], pp.mhi[pi]);
  }
  return p;
}
template <int OBM>
__device__ inline float coef_item(const Geo& g, const Params& pp, int og, int lnob, float inv_nbw, int i, int idx) {
  const int col = idx & ((16 << lnob) - 1), jk = idx >> (4 + lnob);
  const int j = fdiv(jk, g.nbw, inv_nbw), k = jk - j * g.nbw;
  const int o = og * OBM * 16 + col;
  return (o < g.Opad) ? pp.coef[pidx(g, i, j, k, o)] : 0.f;
}
// index of this lane's weight fragment (slice k, output block ob, K-step ks) in a tile's wt[k][ob][ks][64]
template <int KS>
__device__ inline int wk_idx(int k, int NOB, int ob, int ks, int l) { return ((k * NOB + ob) * KS + ks) * 64 + l; }
// The ADC of one partial sum on the unrolled (ballot) paths: the output term, and with state words (WST) the three
// state masks -- STE pass, code != 0, code < 0 -- which the caller shifts in in the order its format needs.
struct AdcMasks { uint64_t mps, mnz, mlo; };
template <bool WST>
__device__ inline AdcMasks ballot_adc(int ps, int4 pv, float cf, float& acc) {
  const uint64_t mhi = __builtin_amdgcn_ballot_w64(ps >= pv.x);
  const uint64_t mlo = __builtin_amdgcn_ballot_w64(ps <= pv.y);
  acc += adc3(cf, mhi, mlo);
  if constexpr (!WST) return AdcMasks{0ull, 0ull, 0ull};  // (no state words -- and none of their bits)
  const uint64_t mps = __builtin_amdgcn_ballot_w64((unsigned)(ps - pv.z) <= (unsigned)pv.w);
  return AdcMasks{mps, mhi | mlo, mlo};
}
// The per-pair loop's state bits of one row: pair (k, j)'s three bits sb (st_bits' order) into weight slice k's
// word stw (interleaved words, the w4a4 word pair) or its three plane words tq (PLF: w8a8)
template <bool PLF>
__device__ inline void add_bits(uint32_t& stw, uint32_t (&tq)[3], int j, uint32_t sb) {
  if (PLF) {
    tq[0] |= (sb & 1u) << j;
    tq[1] |= ((sb >> 1) & 1u) << j;
    tq[2] |= ((sb >> 2) & 1u) << j;
  } else {
    stw |= sb << (3 * j);
  }
}

// CST: compact state words (cimq_v7.hip) -- one uint32 per (tile i, pixel m, channel o) at
// st32[(i*M + m)*O + o], bits 3*(k*nba + j) + {0: STE pass, 1: code != 0, 2: code < 0}; 0: the per-k words.
// CST > 0 also fixes nbw = nba = CST at compile time: the ternary-threshold path then runs
// fully unrolled (every slice pair's MFMAs issued before its ADC work, state bits shifted in).
// CST 4 (w4a4 in 1-bit slices): 16 pairs in a uint2 per (i, m, o) at st64[(i*M + m)*O + o] -- .x the pairs of
// weight slices 0-1 as above (kj 0..7), .y those of slices 2-3 at 3*(kj - 8); its unrolled path agrees with CST 0
// bit for bit.  Its stateless form (ST NONE: the forward-only module calls, v7_w44_eval) is that path without the
// words, their bits and the ballots that feed only them, with the quantiser in the row staging as in CST 2 / 3.
// ST: what becomes of those words (FwdState).  M: what the store does (FwdMode) -- the epilogue ep on the float4
// about to be stored (NCHW only); with codes, the row staging reads the input's codes (ep.xq: bytes straight into
// the word table, stage_rows_qc) or quantises fp32 x as before, and the store writes the float4, the consumer's
// codes (ep.oq) or both; the view costs four scalar loads per float4 and, inside the code instances, a wave per
// SIMD of <4, 1, 0, WRITE, CODES, 2> (96 -> 97 VGPRs): hence instances of its own.
// xin (module path, NBP 4): the activation quantiser fused into the row staging (stage_rows_q)
// Q8 (NBP 8, forward only with an epilogue; a layer of a cimq_net_forward_ex plan alone): the w8a8 layer's row staging
// quantises fp32 xin itself (stage_rows_q8: the prologue's act_words, element by element), so a prepared call is one
// launch; every other instance is what it was
template <int NBP, int KS, int CST, FwdState ST, FwdMode M, int OBM, bool Q8 = false>
__global__ __launch_bounds__(256) void cim_fwd_v3_kernel(Geo g, V3 v, const uint8_t* __restrict__ xcf,
                                                         const v4i* __restrict__ wfrag, Params pp,
                                                         const float* __restrict__ sw_p,
                                                         const float* __restrict__ sa_p, float* __restrict__ out,
                                                         uint8_t* __restrict__ st, const float* __restrict__ xin,
                                                         const float* __restrict__ sgn_p, uint8_t* __restrict__ xcb,
                                                         Epi ep) {
  constexpr bool VIEW = has_view(M), COD = has_codes(M), EPI = has_epi(M);
  constexpr bool WST = ST == FwdState::WRITE, INF = ST == FwdState::NONE;
  static_assert(CST == 0 || CST == 2 || CST == 3 || CST == 4 || CST == 8,
                "state formats: per-k words, w2a2, w3a3, w4a4 word pairs, w8a8 planes");
  static_assert(CST != 4 || (NBP == 4 && ((WST && M == FwdMode::TRAIN) || INF)),
                "w4a4 word pairs: the training forward writes them, every forward-only mode is stateless");
  static_assert(CST != 0 || WST, "CST 0 writes no state words as it is: one form, spelled WRITE, for every call");
  static_assert(ST != FwdState::RECOMPUTE || CST == 8, "the recomputing backward is the w8a8 first conv's");
  static_assert(M != FwdMode::TRAIN || !INF, "a training instance leaves the backward its words, or recomputes them");
  static_assert(M != FwdMode::INFER || INF, "forward only is the stateless form of a compact format");
  static_assert(!EPI || CST == 0 || !WST, "the epilogue instances are forward only");
  static_assert(!Q8 || (NBP == 8 && (CST == 8 || CST == 0) && M == FwdMode::EPI),
                "the staged w8a8 quantiser is an epilogue instance's: the one-block format (CST 8) or per-k (CST 0)");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int og = blockIdx.y;
  const int NOB = min(OBM, g.OB16);
  const int nob = min(OBM, g.OB16 - og * OBM);
  const int TT = v.fwd_res ? g.T : 1;
  const int nkj = g.nbw * g.nba;
  uint8_t* cur = smem;
#define X(name, bytes) uint8_t* const l_##name = cur; cur += bytes;
  CIMQ_FWD3_LDS(X)
#undef X
  uint8_t* patch = l_patch;
  int* ptab = reinterpret_cast<int*>(l_ptab);
  v4i* wfl = reinterpret_cast<v4i*>(l_wfl);
  int4* prm = reinterpret_cast<int4*>(l_prm);
  float* cfl = reinterpret_cast<float*>(l_cfl);
  float* ckl = reinterpret_cast<float*>(l_ckl);
  uint32_t* alut = reinterpret_cast<uint32_t*>(cur);  // the quantiser's word table, after the list

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, g4 = lane >> 4;
  const float sw = *sw_p, sa = *sa_p;
  const bool flag_lit = (pp.flags[0] != 0);
  const bool literal = flag_lit || g.mode != ADC_TERNARY;
  const bool has_code = (g.mode == ADC_SIGN || g.mode == ADC_TERNARY);
  const int Wo = 1 << v.lw;
  // index math by shifts (NOB in {1, 2, 4}, KS in {1, 2}) and a float-reciprocal division
  // by nbw: integer division is ~30 VALU each, and this prologue runs once per block
  const int lnob = NOB == 4 ? 2 : NOB - 1;
  const float inv_nbw = 1.f / (float)g.nbw;
  // the ADC thresholds and coefficients of tile i (the weight side's small part)
  auto stage_prm = [&](int i, int tt) {
    if (!flag_lit) {
      batched_copy<2>(nkj * NOB * 16, prm + (size_t)tt * nkj * NOB * 16,
                      [&](int idx) -> int4 { return thr_item<OBM>(g, pp, og, lnob, inv_nbw, i, idx); });
      batched_copy<4>(nkj * NOB * 16, cfl + (size_t)tt * nkj * NOB * 16,
                      [&](int idx) -> float { return coef_item<OBM>(g, pp, og, lnob, inv_nbw, i, idx); });
    }
  };
  auto stage_tile = [&](int i, int tt) {
    batched_copy<4>(g.nbw * NOB * KS * 64, wfl + (size_t)tt * g.nbw * NOB * KS * 64,
                    [&](int idx) -> v4i { return frag_item<KS, OBM>(g, wfrag, og, nob, lnob, i, idx); });
    stage_prm(i, tt);
  };
  // every tile's weight side at once (fwd_res): one batched pass per array over all tiles, so its
  // loads are in flight together (tile by tile it took T x 3 dependent round trips: 8-9 us of a
  // 40-45 us launch on the 16x16 / 8x8 layers)
  auto stage_all = [&]() {
    const int nw = g.nbw * NOB * KS * 64, np = nkj * NOB * 16;
    const float inv_nw = 1.f / (float)nw, inv_np = 1.f / (float)np;
    batched_copy<8>(g.T * nw, wfl, [&](int t) -> v4i {
      const int i = fdiv(t, nw, inv_nw), idx = t - i * nw;
      return frag_item<KS, OBM>(g, wfrag, og, nob, lnob, i, idx);
    });
    if (!flag_lit) {
      batched_copy<8>(g.T * np, prm, [&](int t) -> int4 {
        const int i = fdiv(t, np, inv_np), idx = t - i * np;
        return thr_item<OBM>(g, pp, og, lnob, inv_nbw, i, idx);
      });
      batched_copy<8>(g.T * np, cfl, [&](int t) -> float {
        const int i = fdiv(t, np, inv_np), idx = t - i * np;
        return coef_item<OBM>(g, pp, og, lnob, inv_nbw, i, idx);
      });
    }
  };

  // non-resident tiles with a compile-time slice count (CST > 0): the next tile's weight fragments
  // are loaded into registers while the current tile computes and stored after the tile barrier
  // (the 16x16 / 8x8 layers, whose tiles do not all fit in LDS, spent 8-9 us per launch staging
  // them tile by tile); the thresholds are still staged at the barrier (in registers too they cost
  // the 32-channel layers a wave per SIMD)
  constexpr int PFW = CST > 0 ? (CST * OBM * KS * 64 + 255) / 256 : 1;
  const bool pfx = CST > 0 && !v.fwd_res && v.pf && blockDim.x == 256;  // uniform
  v4i pw[PFW];
  auto load_tile = [&](int i) {
    const int nw = g.nbw * NOB * KS * 64;
#pragma unroll
    for (int u = 0; u < PFW; ++u) {
      const int idx = threadIdx.x + u * 256;
      pw[u] = v4i{0, 0, 0, 0};
      if (idx < nw) pw[u] = frag_item<KS, OBM>(g, wfrag, og, nob, lnob, i, idx);
    }
  };
  auto store_tile = [&]() {
    const int nw = g.nbw * NOB * KS * 64;
#pragma unroll
    for (int u = 0; u < PFW; ++u)
      if ((int)threadIdx.x + u * 256 < nw) wfl[threadIdx.x + u * 256] = pw[u];
  };
  for (int i = 0; i < g.T; ++i) build_ptab(g, i, KS, v.RH, v.WP, ptab + i * KS * 64);
  for (int t = threadIdx.x; t < 3 * nkj; t += blockDim.x) ckl[t] = pp.ckj[t];
  if (pfx) load_tile(0);  // in flight through the prologue and the first row staging
  if (v.fwd_res) stage_all();
  zero_lds(reinterpret_cast<uint32_t*>(patch), g.C * v.RH * v.WP * NBP / 4);
  const uint8_t* xq = nullptr;
  if constexpr (COD && NBP == 4) xq = ep.xq;
  const bool actq = NBP == 4 && (xin != nullptr || xq != nullptr);  // uniform
  const float sa_q = actq ? *sa_p : 0.f;
  const bool sgn_q = actq && *sgn_p != 0.f;
  // (a compile-time slice count also fixes 1-bit activation slices: CST counts slices, whatever their width, so
  // wider ones take the runtime digit loop; g.bsa is uniform, and either call syncs the block)
  // (CST 4 stages the quantiser in its stateless form only: the training instance keeps the runtime table)
  constexpr int LQ = (CST == 2 || CST == 3 || (CST == 4 && INF)) ? CST : 0;
  if (actq) {
    if (LQ > 0 && g.bsa == 1)
      act_lut_build_q<LQ>(g, sa_q, sgn_q, alut);
    else
      act_lut_build_q<0>(g, sa_q, sgn_q, alut);
  }

  __syncthreads();
  // w8a8: is binary_mask the standard int8-wrapped one (zero exactly where j + k >= 8)?
  const bool std8 = CST != 8 ||
                    __builtin_amdgcn_ballot_w64(lane < nkj && ((ckl[lane < nkj ? lane : 0] != 0.f) != ((lane >> 3) + (lane & 7) < 8))) == 0ull;
  const int pl = wave * 16 + r16;  // this lane's gather pixel within the m-tile
  const int rb = ((pl >> v.lw) * g.SH) * v.WP + (pl & (Wo - 1)) * g.SW;
  const int tiles_per_img = g.P >> 6;
  const float inv_tpi = 1.f / (float)tiles_per_img, inv_p = 1.f / (float)g.P;
  for (int mt = blockIdx.x; mt < v.nmt; mt += gridDim.x) {
    const int b = fdiv(mt, tiles_per_img, inv_tpi), p0 = (mt - b * tiles_per_img) * 64;
    const int oh0 = p0 >> v.lw;
    __syncthreads();
    if constexpr (Q8) {
      stage_rows_q8(g, v.WP, v.RH, xin, *sa_p, *sgn_p != 0.f, b, oh0 * g.SH - g.PH, patch);
    } else if (actq) {
      // input rows this m-tile owns (written once to xcb): its output rows' stride-spans, to the
      // image's end for its last m-tile; one o-group's blocks write them
      const int own_lo = blockIdx.y == 0 ? oh0 * g.SH : 0;
      const int own_hi = blockIdx.y == 0 ? (p0 + 64 == g.P ? g.H : (oh0 + (64 >> v.lw)) * g.SH) : 0;
      if (COD && xq)
        stage_rows_qc(g, v.WP, v.RH, xq, alut, b, oh0 * g.SH - g.PH, patch);
      else if constexpr (NBP == 4)
        stage_rows_q<!INF>(g, v.WP, v.RH, xin, sa_q, alut, b, oh0 * g.SH - g.PH, patch, xcb, own_lo, own_hi);
    } else {
      stage_rows<NBP>(g, v.WP, v.RH, xcf, b, oh0 * g.SH - g.PH, patch);
    }
    __syncthreads();
    float acc[OBM][4];
#pragma unroll
    for (int a = 0; a < OBM; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[a][c] = 0.f;
    for (int i = 0; i < g.T; ++i) {  // per tile: weight side (non-resident tiles), gather, pairs, store state
      if (!v.fwd_res) {
        __syncthreads();
        if (pfx) {
          // the weight fragments from the registers loaded a tile ago; the ADC thresholds as before
          store_tile();
          stage_prm(i, 0);
          load_tile(i + 1 < g.T ? i + 1 : 0);  // the next tile (tile 0 again for the next m-tile)
        } else {
          stage_tile(i, 0);
        }
        __syncthreads();
      }
      const int tt = v.fwd_res ? i : 0;
      const int ksn = (min(g.xbar, g.K - i * g.xbar) + 63) >> 6;  // K-steps holding data in tile i
      v4i xs[NBP][KS];
      // (the fast path runs every K-step: ptab and the weight operand are zero past the tile)
      gather_xs<NBP, KS>(patch, rb, ptab + i * KS * 64, g4, xs, (CST > 0 && !literal && std8) ? KS : ksn);
      const v4i* wt = wfl + (size_t)tt * g.nbw * NOB * KS * 64;
      const int4* pt = prm + (size_t)tt * nkj * NOB * 16;
      const float* ct = cfl + (size_t)tt * nkj * NOB * 16;
      uint32_t stc[OBM][4];
#pragma unroll
      for (int a = 0; a < OBM; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) stc[a][c] = 0u;
      uint32_t stc2[CST == 4 ? OBM : 1][4];  // (CST 4: the word of weight slices 2-3)
      if constexpr (CST == 4) {
#pragma unroll
        for (int a = 0; a < OBM; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c) stc2[a][c] = 0u;
      }
      // plane state words (more than 10 slice pairs, NBP 8): per (i, m, o) three 64-bit planes
      // -- STE pass, code != 0, code < 0 -- bit k*nba + j each (cimq_v7.hip)
      constexpr bool PLF = (NBP == 8) && CST;
      uint64_t pl[OBM][4][3];
#pragma unroll
      for (int a = 0; a < OBM; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) pl[a][c][0] = pl[a][c][1] = pl[a][c][2] = 0ull;
      if constexpr (CST == 4) {
        // pairs, path 1 of 3 -- w4a4 unrolled: the 16 pairs in CST 0's order of additions, k ascending, per output
        // block the four pairs' MFMAs, then j ascending.  Each word takes its 8 pairs' bits from the bottom -- pass,
        // code != 0, code < 0 -- which leaves pair kj's at 23 - 3*(kj & 7) - {0, 1, 2}: a bit reversal and a shift by
        // 8 put them at 3*(kj & 7) + {0, 1, 2}, where cimq_v7.hip reads them.
        if (!literal) {
          uint32_t sh[OBM][4][2];
#pragma unroll
          for (int a = 0; a < OBM; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) sh[a][c][0] = sh[a][c][1] = 0u;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int ob = 0; ob < OBM; ++ob) {
              if (ob < nob) {
                v4i wk[KS];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) wk[ks] = wt[wk_idx<KS>(k, NOB, ob, ks, lane)];
                v4i ps[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                  ps[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(xs[j][0], wk[0], v4i{0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
                  for (int ks = 1; ks < KS; ++ks) ps[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(xs[j][ks], wk[ks], ps[j], 0, 0, 0);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                  const int pcol = (j * 4 + k) * NOB * 16 + ob * 16 + r16;
                  const int4 pv = pt[pcol];
                  const float cf = ct[pcol];
#pragma unroll
                  for (int r = 0; r < 4; ++r) {
                    const AdcMasks m = ballot_adc<WST>(ps[j][r], pv, cf, acc[ob][r]);
                    if constexpr (!WST) continue;
                    sh[ob][r][k >> 1] = shin(shin(shin(sh[ob][r][k >> 1], m.mps), m.mnz), m.mlo);
                  }
                }
              }
            }
          }
#pragma unroll
          for (int a = 0; a < OBM; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              if constexpr (!WST) continue;
              stc[a][c] = __builtin_bitreverse32(sh[a][c][0]) >> 8;
              stc2[CST == 4 ? a : 0][c] = __builtin_bitreverse32(sh[a][c][1]) >> 8;
            }
        }
      } else if (CST > 0 && !literal && std8) {
        // pairs, path 2 of 3 -- compact unrolled: slice pairs kj = k*CST + j in descending order, so that
        // shifting each state bit in from the bottom leaves bit 3*kj + {0,1,2} (interleaved words) or bit
        // kj of each 64-bit plane (PLF) where cimq_v7.hip reads it.  w8a8 (CST 8) runs it only
        // with the standard int8-wrapped binary_mask (_quan_base.py:207-214), whose pairs with
        // j + k >= 8 are 0: they add adc * 0 = 0 to the output and G * 0 = 0 to every gradient,
        // so neither their MFMAs nor their ADC run and their state bits stay 0 (exact: this path
        // has finite ADC outputs).  Any other mask takes the per-pair loop below.
        constexpr int NS = CST > 0 ? CST : 1;
        uint32_t sw3[OBM][4][PLF ? 6 : 1];
#pragma unroll
        for (int a = 0; a < OBM; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int q = 0; q < (PLF ? 6 : 1); ++q) sw3[a][c][q] = 0u;
#pragma unroll
        for (int k = NS - 1; k >= 0; --k) {
#pragma unroll
          for (int ob = 0; ob < OBM; ++ob) {
            if (ob < nob) {
              v4i wk[KS];
#pragma unroll
              for (int ks = 0; ks < KS; ++ks) wk[ks] = wt[wk_idx<KS>(k, NOB, ob, ks, lane)];
              v4i ps[NS];
#pragma unroll
              for (int j = 0; j < NS; ++j) {
                if (CST != 8 || j + k < 8) {  // compile time once unrolled (w8a8: standard mask only)
                  // (the first K-step from the inline zero accumulator: no register clearing)
                  ps[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(xs[j][0], wk[0], v4i{0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
                  for (int ks = 1; ks < KS; ++ks) ps[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(xs[j][ks], wk[ks], ps[j], 0, 0, 0);
                } else {
                  ps[j] = v4i{0, 0, 0, 0};  // (a mask-0 pair: never read)
                }
              }
#pragma unroll
              for (int j = NS - 1; j >= 0; --j) {
                const int kj = k * NS + j;
                if (CST == 8 && j + k >= 8) {  // mask-0 pair of the wrapped 8-bit mask: zero state bits
#pragma unroll
                  for (int r = 0; r < 4; ++r) {
                    if constexpr (!WST) continue;
                    if constexpr (PLF) {
                      const int wd = kj >= 32 ? 1 : 0;
                      sw3[ob][r][wd] <<= 1;
                      sw3[ob][r][2 + wd] <<= 1;
                      sw3[ob][r][4 + wd] <<= 1;
                    } else {
                      sw3[ob][r][0] <<= 3;
                    }
                  }
                  continue;
                }
                const int pcol = (j * NS + k) * NOB * 16 + ob * 16 + r16;
                const int4 pv = pt[pcol];
                const float cf = ct[pcol];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  const AdcMasks m = ballot_adc<WST>(ps[j][r], pv, cf, acc[ob][r]);
                  if constexpr (!WST) continue;
                  if constexpr (PLF) {
                    const int wd = kj >= 32 ? 1 : 0;
                    sw3[ob][r][wd] = shin(sw3[ob][r][wd], m.mps);
                    sw3[ob][r][2 + wd] = shin(sw3[ob][r][2 + wd], m.mnz);
                    sw3[ob][r][4 + wd] = shin(sw3[ob][r][4 + wd], m.mlo);
                  } else {
                    sw3[ob][r][0] = shin(shin(shin(sw3[ob][r][0], m.mlo), m.mnz), m.mps);
                  }
                }
              }
            }
          }
        }
#pragma unroll
        for (int a = 0; a < OBM; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            if constexpr (PLF) {
#pragma unroll
              for (int q = 0; q < 3; ++q)
                pl[a][c][q] = (uint64_t)sw3[a][c][2 * q] | ((uint64_t)sw3[a][c][2 * q + 1] << 32);
            } else {
              stc[a][c] = sw3[a][c][0];
            }
          }
      }
      // pairs, path 3 of 3 -- the per-k loop: every format and ADC flavour, run-time slice counts
      for (int k = 0; k < ((CST > 0 && !literal && std8) ? 0 : g.nbw); ++k) {
#pragma unroll
        for (int ob = 0; ob < OBM; ++ob) {
          if (ob < nob) {
            const int o = (og * OBM + ob) * 16 + r16;
            v4i wk[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) wk[ks] = wt[wk_idx<KS>(k, NOB, ob, ks, lane)];
            uint32_t stw[4] = {0u, 0u, 0u, 0u};
            uint32_t tq[4][3] = {{0u, 0u, 0u}, {0u, 0u, 0u}, {0u, 0u, 0u}, {0u, 0u, 0u}};
#pragma unroll
            for (int j = 0; j < NBP; ++j) {
              if (j < g.nba) {
                v4i ps = {0, 0, 0, 0};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) if (ks < ksn) ps = __builtin_amdgcn_mfma_i32_16x16x64_i8(xs[j][ks], wk[ks], ps, 0, 0, 0);
                const int pcol = (j * g.nbw + k) * NOB * 16 + ob * 16 + r16;
                if (!literal) {
                  const int4 pv = pt[pcol];
                  const float cf = ct[pcol];
#pragma unroll
                  for (int r = 0; r < 4; ++r) {
                    const bool hi = ps[r] >= pv.x, lo = ps[r] <= pv.y;
                    float a = hi ? cf : 0.f;
                    a = lo ? -cf : a;
                    acc[ob][r] += a;
                    if constexpr (INF) continue;  // (forward only: no state bits)
                    const bool pass = (unsigned)(ps[r] - pv.z) <= (unsigned)pv.w;
                    add_bits<PLF>(stw[r], tq[r], j, (pass ? 1u : 0u) | ((hi || lo) ? 2u : 0u) | (lo ? 4u : 0u));
                  }
                } else if (is_shift(g)) {
                  const float al = pp.alpha[pidx(g, i, j, k, o)], be = pp.beta[pidx(g, i, j, k, o)];
                  const float mk = ckl[k * g.nba + j];
#pragma unroll
                  for (int r = 0; r < 4; ++r) {
                    acc[ob][r] += shift_adc_literal(ps[r], sw, sa, al, be, mk);
                    if constexpr (INF) continue;
                    add_bits<PLF>(stw[r], tq[r], j, shift_state_literal(ps[r], sw, sa, al, be, g.thr_hi, g.thr_lo));
                  }
                } else {
                  const float al = pp.alpha[pidx(g, i, j, k, o)];
                  const float mk = ckl[k * g.nba + j];
                  const int4 pv = pt[pcol];
#pragma unroll
                  for (int r = 0; r < 4; ++r) {
                    acc[ob][r] += adc_literal_sum(ps, g.mode, sw, sa, al, g.qn, g.qp, mk, r);
                    if constexpr (INF) continue;
                    const bool pass = flag_lit ? (ste_literal(ps[r], g.mode, sw, sa, al, g.thr_hi, g.thr_lo) != 0.f)
                                               : ((unsigned)(ps[r] - pv.z) <= (unsigned)pv.w);
                    const float code =
                        has_code ? code_literal(ps[r], g.mode, sw, sa, al, g.qn, g.qp, g.thr_hi, g.thr_lo) : 0.f;
                    add_bits<PLF>(stw[r], tq[r], j, st_bits(pass, code));
                  }
                }
              }
            }
            if (PLF) {
#pragma unroll
              for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int q = 0; q < 3; ++q) pl[ob][r][q] |= (uint64_t)tq[r][q] << (g.nba * k);
            } else if constexpr (CST == 4) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                if (k < 2) stc[ob][r] |= stw[r] << (12 * k);
                else stc2[CST == 4 ? ob : 0][r] |= stw[r] << (12 * (k - 2));
              }
            } else if (CST) {
#pragma unroll
              for (int r = 0; r < 4; ++r) stc[ob][r] |= stw[r] << (3 * g.nba * k);
            }
          }
        }
      }
      if (CST && WST) {  // store state: the words in their format's layout
#pragma unroll
        for (int ob = 0; ob < OBM; ++ob) {
          const int o = (og * OBM + ob) * 16 + r16;
          if (ob < nob && o < g.O) {
            const size_t e0 = ((size_t)i * g.M + (size_t)mt * 64 + wave * 16 + 4 * g4) * g.O + o;
            if constexpr (CST == 4) {
              uint2* s64 = reinterpret_cast<uint2*>(st) + e0;
#pragma unroll
              for (int r = 0; r < 4; ++r) s64[(size_t)r * g.O] = make_uint2(stc[ob][r], stc2[CST == 4 ? ob : 0][r]);
            } else if (PLF) {
              uint2* s64 = reinterpret_cast<uint2*>(st);
#pragma unroll
              for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int q = 0; q < 3; ++q)
                  s64[(e0 + (size_t)r * g.O) * 3 + q] = make_uint2((uint32_t)pl[ob][r][q], (uint32_t)(pl[ob][r][q] >> 32));
            } else {
              uint32_t* s32 = reinterpret_cast<uint32_t*>(st) + e0;
#pragma unroll
              for (int r = 0; r < 4; ++r) s32[(size_t)r * g.O] = stc[ob][r];
            }
          }
        }
      }
    }
    // store out, its mode branches in one place.  acc[ob][r]: pixel wave*16 + 4*g4 + r, channel (og*OBM + ob)*16 + r16
#pragma unroll
    for (int ob = 0; ob < OBM; ++ob) {
      const int o = (og * OBM + ob) * 16 + r16;
      if (ob < nob && o < g.O) {
        if (is_shift(g) && !literal) {
          // the threshold path sums code * alpha * mask; the shift ADC adds beta * mask per pair
          const float bs = pp.bsum[o];
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[ob][r] += bs;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (!g.onchw) out[((size_t)mt * 64 + wave * 16 + 4 * g4 + r) * g.O + o] = acc[ob][r];
        if (g.onchw) {
          const int m4 = mt * 64 + wave * 16 + 4 * g4;  // M < 2^24 (v3_plan)
          const int bb = fdiv(m4, g.P, inv_p), pq = m4 - bb * g.P;
          const size_t oi = ((size_t)bb * g.O + o) * g.P + pq;
          if constexpr (EPI) {
            // (the table index through an opaque copy: the two 64-bit entry addresses, invariant over the m-tiles,
            // would otherwise be kept in 4 VGPRs per output block across the whole loop -- a wave per SIMD in the
            // OBM 4 instances)
            int oe = o;
            asm volatile("" : "+v"(oe));
            float4 v4;
            if constexpr (VIEW)
              v4 = epi_val4v(ep, ep.scale[oe], ep.shift[oe], oi, bb, oe, pq, g.Wo, acc[ob][0], acc[ob][1], acc[ob][2],
                             acc[ob][3]);
            else
              v4 = epi_val4(ep, ep.scale[oe], ep.shift[oe], oi, acc[ob][0], acc[ob][1], acc[ob][2], acc[ob][3]);
            if constexpr (COD) store_codes4(ep, out, oi, v4);
            else *reinterpret_cast<float4*>(out + oi) = v4;
          } else
            *reinterpret_cast<float4*>(out + oi) = make_float4(acc[ob][0], acc[ob][1], acc[ob][2], acc[ob][3]);
        }
      }
    }
  }
}

}  // namespace cimq
