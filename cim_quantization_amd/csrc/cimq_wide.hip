// cimq_wide.hip -- the forward of a module-path (NCHW out) layer whose input channels do not fit
// cim_fwd_v3_kernel's whole-C LDS patch (wide_plan: C >= 128; VGG7's 3x3 layers from 128 channels up).
//
// Same pixel geometry as cim_fwd_v3_kernel -- a 256-thread workgroup owns one 64-pixel whole-row m-tile
// (grid-stride) x up to four 16-channel output blocks (blockIdx.y), wave w gathers pixels 16w .. 16w+15 straight
// from the LDS patch -- but the patch holds one *channel chunk* at a time: channels [c0, c0 + ncx) for a run of
// WideP::tr consecutive crossbar tiles, c0 = floor(i0 * xbar / KHW) for the run's first tile i0, so neighbouring
// chunks share the boundary channel of a tile that straddles it.  The weight side is v3's non-resident form: one
// tile's fragments, thresholds and coefficients in LDS, the next tile's fragments in flight in registers.
//
// Order of additions into the fp32 accumulators acc[ob][r], which live across all tiles: tile i ascending, then
// weight slice k ascending, then activation slice j ascending -- cim_fwd_v3_kernel's order.
//
// No state words, in any mode: a wide layer's backward is the general one, which recomputes the partial sums from
// the prologue's ctx words.  TRAIN reads the prologue's forward slice words (xcode); INFER and EPI read fp32 x and
// quantise it in the row staging with stage_rows_q's table and element chain, so a prepared forward-only layer is
// one launch.
#include "cimq_kernels_v3.hip"

namespace cimq {

// stage_rows_q<false> over the channel window [c0, c0 + ncx): patch row (c - c0, rr) <- image row ih_first + rr of
// channel c, each element through act_words_tab (the words are the prologue's bit for bit)
__device__ inline void stage_rows_qw(const Geo& g, int WP, int RHx, const float* __restrict__ x, float sa,
                                     const uint32_t* lut, int b, int ih_first, uint8_t* patch, int c0, int ncx) {
  const int nan_e = (int)g.lsq_qp + 1;
  const int QW = g.W >> 2;  // 4-element items per row (W % 4 == 0)
  const int nrow = ncx * RHx;
  const int n = nrow * QW;
  const bool pq = (QW & (QW - 1)) == 0;
  const int lq = 31 - __builtin_clz(QW);
  const float invQ = 1.f / (float)QW, invR = 1.f / (float)RHx;
  const float4* src = reinterpret_cast<const float4*>(x) + ((size_t)b * g.C + c0) * g.H * QW;
  const int HQ = g.H * QW;
  for (int base = threadIdx.x; base < n; base += 4 * (int)blockDim.x) {
    float4 v[4];
    int d[4];
    bool in[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = base + u * (int)blockDim.x;
      d[u] = -1;
      in[u] = false;
      v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (idx < n) {
        const int row = pq ? (idx >> lq) : fdiv(idx, QW, invQ), q = pq ? (idx & (QW - 1)) : idx - row * QW;
        const int c = fdiv(row, RHx, invR);
        const int ih = ih_first + (row - c * RHx);
        d[u] = row * WP * 4 + g.PW * 4 + q * 16;
        in[u] = (unsigned)ih < (unsigned)g.H;
        if (in[u]) v[u] = src[c * HQ + ih * QW + q];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (d[u] < 0) continue;
      uint32_t* p = reinterpret_cast<uint32_t*>(patch + d[u]);
      if (!in[u]) {
        p[0] = p[1] = p[2] = p[3] = 0u;
        continue;
      }
      p[0] = act_words_tab(v[u].x, sa, g.lsq_qp, nan_e, lut).x;
      p[1] = act_words_tab(v[u].y, sa, g.lsq_qp, nan_e, lut).x;
      p[2] = act_words_tab(v[u].z, sa, g.lsq_qp, nan_e, lut).x;
      p[3] = act_words_tab(v[u].w, sa, g.lsq_qp, nan_e, lut).x;
    }
  }
}

// torch's max-pool update (max_pool_forward_nchw: v > m || isnan(v)) on an ordered pair: the earlier element m stays
// unless the later one is greater or a NaN -- so any NaN gives NaN and of +0 / -0 the earlier wins.  Compare and
// select: v_max_f32 drops NaNs and does not order the zeros.  pool_pick(pool_pick(a, b), pool_pick(c, d)) is the
// sequential scan a, b, c, d bit for bit.
__device__ inline float pool_pick(float m, float v) { return (v > m || v != v) ? v : m; }

// CST: 2 / 3 / 4 fix nbw = nba = CST in 1-bit slices at compile time (the ternary-threshold path then runs
// unrolled); 0 takes the counts -- and slices of any width -- at run time.  M: TRAIN, INFER or EPI (FwdMode).
// POOL (EPI alone): the epilogue's values leave through a 2x2 / stride-2 max pool, out is [B, O, Ho/2, Wo/2] -- see
// pool_pick and the store below (wide_pool_ok on the host: Wo <= 32, so that both rows of a window sit in one m-tile).
template <int KS, int CST, FwdMode M, bool POOL = false>
__global__ __launch_bounds__(256) void cim_fwd_wide_kernel(Geo g, V3 v, WideP wp, const uint8_t* __restrict__ xcf,
                                                           const v4i* __restrict__ wfrag, Params pp,
                                                           const float* __restrict__ sw_p,
                                                           const float* __restrict__ sa_p, float* __restrict__ out,
                                                           const float* __restrict__ xin,
                                                           const float* __restrict__ sgn_p, Epi ep) {
  constexpr int NBP = 4, OBM = kWideOBM, NOB = kWideOBM, lnob = 2;
  constexpr bool EPI = has_epi(M), ACTQ = M != FwdMode::TRAIN;
  static_assert(M == FwdMode::TRAIN || M == FwdMode::INFER || M == FwdMode::EPI, "codes and views are not built");
  static_assert(CST == 0 || CST == 2 || CST == 3 || CST == 4, "runtime counts, or w2a2 / w3a3 / w4a4 in 1-bit slices");
  static_assert(!POOL || M == FwdMode::EPI, "the pooled store is the epilogue instances' alone");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int og = blockIdx.y;
  const int nob = min(OBM, g.OB16 - og * OBM);
  const int nkj = g.nbw * g.nba;
  uint8_t* cur = smem;
#define X(name, bytes) uint8_t* const l_##name = cur; cur += bytes;
  CIMQ_WIDE_LDS(X)
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
  const int Wo = 1 << v.lw;
  const float inv_nbw = 1.f / (float)g.nbw;
  const int nw = g.nbw * NOB * KS * 64;  // one tile's weight fragments
  auto stage_prm = [&](int i) {
    if (!flag_lit) {
      batched_copy<2>(nkj * NOB * 16, prm, [&](int idx) -> int4 { return thr_item<OBM>(g, pp, og, lnob, inv_nbw, i, idx); });
      batched_copy<4>(nkj * NOB * 16, cfl, [&](int idx) -> float { return coef_item<OBM>(g, pp, og, lnob, inv_nbw, i, idx); });
    }
  };
  auto stage_tile = [&](int i) {
    batched_copy<4>(nw, wfl, [&](int idx) -> v4i { return frag_item<KS, OBM>(g, wfrag, og, nob, lnob, i, idx); });
    stage_prm(i);
  };
  // compile-time slice counts: the next tile's weight fragments are loaded into registers while this tile computes
  constexpr int PFW = CST > 0 ? (CST * OBM * KS * 64 + 255) / 256 : 1;
  const bool pfx = CST > 0 && wp.pf && blockDim.x == 256;  // uniform
  v4i pw[PFW];
  auto load_tile = [&](int i) {
#pragma unroll
    for (int u = 0; u < PFW; ++u) {
      const int idx = threadIdx.x + u * 256;
      pw[u] = v4i{0, 0, 0, 0};
      if (idx < nw) pw[u] = frag_item<KS, OBM>(g, wfrag, og, nob, lnob, i, idx);
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int u = 0; u < PFW; ++u)
      if ((int)threadIdx.x + u * 256 < nw) wfl[threadIdx.x + u * 256] = pw[u];
  };
  for (int t = threadIdx.x; t < 3 * nkj; t += blockDim.x) ckl[t] = pp.ckj[t];
  if (pfx) load_tile(0);  // in flight through the prologue and the first row staging
  // (the padding columns stay zero: the row stagings write data columns only)
  zero_lds(reinterpret_cast<uint32_t*>(patch), wp.ncx * v.RH * v.WP);
  float sa_q = 0.f;
  if constexpr (ACTQ) {
    sa_q = *sa_p;
    const bool sgn_q = *sgn_p != 0.f;
    // (a compile-time slice count fixes 1-bit activation slices; either call syncs the block)
    if constexpr (CST > 0) act_lut_build_q<CST>(g, sa_q, sgn_q, alut);
    else act_lut_build_q<0>(g, sa_q, sgn_q, alut);
  }
  __syncthreads();
  const int pl = wave * 16 + r16;  // this lane's gather pixel within the m-tile
  const int rb = ((pl >> v.lw) * g.SH) * v.WP + (pl & (Wo - 1)) * g.SW;
  const int tiles_per_img = g.P >> 6;
  const float inv_tpi = 1.f / (float)tiles_per_img, inv_p = 1.f / (float)g.P;
  for (int mt = blockIdx.x; mt < v.nmt; mt += gridDim.x) {
    const int b = fdiv(mt, tiles_per_img, inv_tpi), p0 = (mt - b * tiles_per_img) * 64;
    const int oh0 = p0 >> v.lw;
    float acc[OBM][4];
#pragma unroll
    for (int a = 0; a < OBM; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[a][c] = 0.f;
    int i0 = 0;  // first tile of the chunk in LDS
    for (int i = 0; i < g.T; ++i) {
      __syncthreads();  // the previous tile's reads of the weight side (and, at a chunk's end, of the patch) are done
      if (i == i0 + wp.tr || i == 0) {
        // the next channel chunk: tiles [i0, i1), channels [c0, c0 + ncr) -- ncr <= WideP::ncx (wide_plan)
        i0 = i;
        const int i1 = min(g.T, i0 + wp.tr);
        const int c0 = (i0 * g.xbar) / g.KHW;
        const int ncr = (min(i1 * g.xbar, g.K) - 1) / g.KHW - c0 + 1;
        if constexpr (ACTQ) stage_rows_qw(g, v.WP, v.RH, xin, sa_q, alut, b, oh0 * g.SH - g.PH, patch, c0, ncr);
        else stage_rows<NBP>(g, v.WP, v.RH, xcf, b, oh0 * g.SH - g.PH, patch, c0, ncr);
        for (int q = i0; q < i1; ++q) build_ptab(g, q, KS, v.RH, v.WP, ptab + (q - i0) * KS * 64, c0);
      }
      if (pfx) {
        store_tile();
        stage_prm(i);
        load_tile(i + 1 < g.T ? i + 1 : 0);  // the next tile (tile 0 again for the next m-tile)
      } else {
        stage_tile(i);
      }
      __syncthreads();
      const int ksn = (min(g.xbar, g.K - i * g.xbar) + 63) >> 6;  // K-steps holding data in tile i
      v4i xs[NBP][KS];
      // (the unrolled path runs every K-step: ptab and the weight operand are zero past the tile)
      gather_xs<NBP, KS>(patch, rb, ptab + (i - i0) * KS * 64, g4, xs, (CST > 0 && !literal) ? KS : ksn);
      if (CST > 0 && !literal) {
        // slice pairs unrolled: per weight slice k and output block the CST pairs' MFMAs, then their ADCs, j ascending
        constexpr int NS = CST > 0 ? CST : 1;
#pragma unroll
        for (int k = 0; k < NS; ++k) {
#pragma unroll
          for (int ob = 0; ob < OBM; ++ob) {
            if (ob < nob) {
              v4i wk[KS];
#pragma unroll
              for (int ks = 0; ks < KS; ++ks) wk[ks] = wfl[wk_idx<KS>(k, NOB, ob, ks, lane)];
              v4i ps[NS];
#pragma unroll
              for (int j = 0; j < NS; ++j) {
                ps[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(xs[j][0], wk[0], v4i{0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
                for (int ks = 1; ks < KS; ++ks) ps[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(xs[j][ks], wk[ks], ps[j], 0, 0, 0);
              }
#pragma unroll
              for (int j = 0; j < NS; ++j) {
                const int pcol = (j * NS + k) * NOB * 16 + ob * 16 + r16;
                const int4 pv = prm[pcol];
                const float cf = cfl[pcol];
#pragma unroll
                for (int r = 0; r < 4; ++r) (void)ballot_adc<false>(ps[j][r], pv, cf, acc[ob][r]);
              }
            }
          }
        }
      } else {
        // the per-pair loop: run-time slice counts, slices of any width, every ADC flavour of the library variant
        for (int k = 0; k < g.nbw; ++k) {
#pragma unroll
          for (int ob = 0; ob < OBM; ++ob) {
            if (ob < nob) {
              const int o = (og * OBM + ob) * 16 + r16;
              v4i wk[KS];
#pragma unroll
              for (int ks = 0; ks < KS; ++ks) wk[ks] = wfl[wk_idx<KS>(k, NOB, ob, ks, lane)];
#pragma unroll
              for (int j = 0; j < NBP; ++j) {
                if (j < g.nba) {
                  v4i ps = {0, 0, 0, 0};
#pragma unroll
                  for (int ks = 0; ks < KS; ++ks) if (ks < ksn) ps = __builtin_amdgcn_mfma_i32_16x16x64_i8(xs[j][ks], wk[ks], ps, 0, 0, 0);
                  if (!literal) {
                    const int pcol = (j * g.nbw + k) * NOB * 16 + ob * 16 + r16;
                    const int4 pv = prm[pcol];
                    const float cf = cfl[pcol];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                      float a = ps[r] >= pv.x ? cf : 0.f;
                      a = ps[r] <= pv.y ? -cf : a;
                      acc[ob][r] += a;
                    }
                  } else {
                    // adc_value's library branch (the plan admits no other variant), out of line as in v3
                    const float al = o < g.Opad ? pp.alpha[pidx(g, i, j, k, o)] : 0.f;
                    const float mk = ckl[k * g.nba + j];
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[ob][r] += adc_literal_sum(ps, g.mode, sw, sa, al, g.qn, g.qp, mk, r);
                  }
                }
              }
            }
          }
        }
      }
    }
    // store out (NCHW).  acc[ob][r]: pixel wave*16 + 4*g4 + r, channel (og*OBM + ob)*16 + r16
    if constexpr (POOL) {
      // The 2x2 / stride-2 max pool of the epilogue's values.  A lane's four pixels are one row's columns 4q' .. 4q' + 3
      // (Wo % 4 == 0): the two horizontal pairs are pooled in registers.  The window's other row is pixel + Wo: the
      // quad (wave * 4 + g4) ^ (Wo / 4) of this m-tile (64 / Wo rows, an even count from an even row: Wo <= 32 and
      // P % 64 == 0).  The lower row's halves go through the weight-fragment region of LDS -- dead after the last
      // tile's MFMAs and rewritten whole by the next m-tile's first store_tile / stage_tile behind the loop's top
      // barrier (the patch is not free: its padding columns are zeroed once per block) -- as one float2 per lane and
      // block, [ob][quad][r16]: consecutive lanes write and read consecutive 8-byte words.  The upper row's lane pools
      // top before bottom, so the result is the first maximal element in the scan order (0,0) (0,1) (1,0) (1,1).
      float2* ex = reinterpret_cast<float2*>(l_wfl);
      const int quad = wave * 4 + g4, qpr = Wo >> 2;
      const bool top = (quad & qpr) == 0;
      const int m4 = mt * 64 + quad * 4;  // M < 2^24 (wide_plan)
      const int bb = fdiv(m4, g.P, inv_p), pq = m4 - bb * g.P;
      float2 hz[OBM];
#pragma unroll
      for (int ob = 0; ob < OBM; ++ob) {
        const int o = (og * OBM + ob) * 16 + r16;
        hz[ob] = make_float2(0.f, 0.f);
        if (ob < nob && o < g.O) {
          const size_t oi = ((size_t)bb * g.O + o) * g.P + pq;  // the unpooled index: the residual's
          int oe = o;
          asm volatile("" : "+v"(oe));
          const float4 y = epi_val4(ep, ep.scale[oe], ep.shift[oe], oi, acc[ob][0], acc[ob][1], acc[ob][2], acc[ob][3]);
          hz[ob] = make_float2(pool_pick(y.x, y.y), pool_pick(y.z, y.w));
        }
      }
      __syncthreads();  // every wave's reads of the last tile's weight fragments are done
      if (!top) {
#pragma unroll
        for (int ob = 0; ob < OBM; ++ob)
          if (ob < nob) ex[(ob * 16 + quad) * 16 + r16] = hz[ob];
      }
      __syncthreads();
      if (top) {
        const int Wh = Wo >> 1, Ph = g.P >> 2;
        const int pp = ((pq >> v.lw) >> 1) * Wh + ((pq & (Wo - 1)) >> 1);  // the pooled pixel of the lane's first window
#pragma unroll
        for (int ob = 0; ob < OBM; ++ob) {
          const int o = (og * OBM + ob) * 16 + r16;
          if (ob < nob && o < g.O) {
            const float2 lo = ex[(ob * 16 + (quad | qpr)) * 16 + r16];
            *reinterpret_cast<float2*>(out + ((size_t)bb * g.O + o) * Ph + pp) =
                make_float2(pool_pick(hz[ob].x, lo.x), pool_pick(hz[ob].y, lo.y));
          }
        }
      }
      continue;  // (the next m-tile's top barrier follows the reads above)
    }
#pragma unroll
    for (int ob = 0; ob < OBM; ++ob) {
      const int o = (og * OBM + ob) * 16 + r16;
      if (ob < nob && o < g.O) {
        const int m4 = mt * 64 + wave * 16 + 4 * g4;  // M < 2^24 (wide_plan)
        const int bb = fdiv(m4, g.P, inv_p), pq = m4 - bb * g.P;
        const size_t oi = ((size_t)bb * g.O + o) * g.P + pq;
        if constexpr (EPI) {
          int oe = o;
          asm volatile("" : "+v"(oe));
          *reinterpret_cast<float4*>(out + oi) =
              epi_val4(ep, ep.scale[oe], ep.shift[oe], oi, acc[ob][0], acc[ob][1], acc[ob][2], acc[ob][3]);
        } else {
          *reinterpret_cast<float4*>(out + oi) = make_float4(acc[ob][0], acc[ob][1], acc[ob][2], acc[ob][3]);
        }
      }
    }
  }
}

}  // namespace cimq
