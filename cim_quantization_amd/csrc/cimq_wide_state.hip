// cimq_wide_state.hip -- the state-writing training forward of a wide module layer (CIMQ_OPT_WIDE_BWD):
// cim_fwd_wide_kernel<KS, CST, TRAIN>'s walk -- the same LDS list (CIMQ_WIDE_LDS), channel chunks, weight-side prefetch
// and, above all, the same order of additions into acc, so out is that kernel's bit for bit -- which also leaves the
// compact state words of cimq_v7.hip: one uint32 (CST 2 / 3) or uint2 (CST 4: .x weight slices 0-1, .y slices 2-3) per
// (tile, pixel, channel) at [T][M][O], bits 3 * kj + {0 STE pass, 1 code != 0, 2 code < 0}, for the channel-chunked
// backward (cimq_wide_bwd.hip).  A kernel of its own and not a mode of cim_fwd_wide_kernel: that kernel's names and
// instruction streams stay what they were (tools/isa_diff.py), and this one carries no forward-only mode, epilogue,
// pool or staged quantiser.  The words are built as cim_fwd_v3_kernel<CST, WRITE> builds them: on the threshold path
// ballot_adc<true>'s three lane masks shifted in from the bottom, pair kj ascending (this kernel's order of additions:
// k, then j), and the word reversed at the end as in v3's w4a4 path; on the literal path (flag_lit) v3's per-pair
// loop with ste_literal / code_literal.  A lane holds four pixels of one channel, so its stores are 4-byte (8-byte)
// words 16 lanes wide: 16-byte stores would need a cross-lane transpose of [pixel][channel].
#include "cimq_wide.hip"

namespace cimq {

template <int KS, int CST>
__global__ __launch_bounds__(256) void cim_fwd_wide_state_kernel(Geo g, V3 v, WideP wp,
                                                                 const uint8_t* __restrict__ xcf,
                                                                 const v4i* __restrict__ wfrag, Params pp,
                                                                 const float* __restrict__ sw_p,
                                                                 const float* __restrict__ sa_p,
                                                                 float* __restrict__ out, uint8_t* __restrict__ st) {
  constexpr int NBP = 4, OBM = kWideOBM, NOB = kWideOBM, lnob = 2;
  static_assert(CST == 2 || CST == 3 || CST == 4, "w2a2 / w3a3 / w4a4 in 1-bit slices");
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
  constexpr int PFW = (CST * OBM * KS * 64 + 255) / 256;
  const bool pfx = wp.pf && blockDim.x == 256;  // uniform
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
        stage_rows<NBP>(g, v.WP, v.RH, xcf, b, oh0 * g.SH - g.PH, patch, c0, ncr);
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
      gather_xs<NBP, KS>(patch, rb, ptab + (i - i0) * KS * 64, g4, xs, (!literal) ? KS : ksn);
      // state words: stc the uint32, or .x of the uint2 whose .y is stc2 (weight slices 2-3)
      uint32_t stc[OBM][4], stc2[CST == 4 ? OBM : 1][4];
      {
#pragma unroll
        for (int a = 0; a < OBM; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            stc[a][c] = 0u;
            if constexpr (CST == 4) stc2[a][c] = 0u;
          }
      }
      if (!literal) {
        // slice pairs unrolled: per weight slice k and output block the CST pairs' MFMAs, then their ADCs, j ascending
        constexpr int NS = CST;
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
                for (int r = 0; r < 4; ++r) {
                  const AdcMasks am = ballot_adc<true>(ps[j][r], pv, cf, acc[ob][r]);
                  // pair kj = k * NS + j ascending, its bits shifted in from the bottom -- pass, code != 0, code < 0:
                  // reversed below (cim_fwd_v3_kernel's w4a4 path), where a word holds the pairs of two weight slices
                  {
                    uint32_t& w = (CST == 4 && k >= 2) ? stc2[CST == 4 ? ob : 0][r] : stc[ob][r];
                    w = shin(shin(shin(w, am.mps), am.mnz), am.mlo);
                  }
                }
              }
            }
          }
        }
        {
          // 3 * pairs bits per word came in from the bottom, the first pair's on top: reversed and shifted down, pair
          // kj's sit at 3 * kj + {0, 1, 2} (kj - 8 in .y), where cimq_v7.hip's decodes read them
          constexpr int SHR = CST == 4 ? 8 : 32 - 3 * NS * NS;
#pragma unroll
          for (int a = 0; a < OBM; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              stc[a][c] = __builtin_bitreverse32(stc[a][c]) >> SHR;
              if constexpr (CST == 4) stc2[a][c] = __builtin_bitreverse32(stc2[a][c]) >> SHR;
            }
        }
      } else {
        // the literal flag (degenerate alpha_cim / scales; the plan takes the ternary ADC alone): v3's per-pair loop with
        // adc_value's library branch out of line, the state bits from ste_literal / code_literal
        for (int k = 0; k < g.nbw; ++k) {
#pragma unroll
          for (int ob = 0; ob < OBM; ++ob) {
            if (ob < nob) {
              const int o = (og * OBM + ob) * 16 + r16;
              v4i wk[KS];
#pragma unroll
              for (int ks = 0; ks < KS; ++ks) wk[ks] = wfl[wk_idx<KS>(k, NOB, ob, ks, lane)];
              uint32_t stw[4] = {0u, 0u, 0u, 0u};  // slice k's bits, 3 * j up: cim_fwd_v3_kernel's per-pair loop
#pragma unroll
              for (int j = 0; j < NBP; ++j) {
                if (j < g.nba) {
                  v4i ps = {0, 0, 0, 0};
#pragma unroll
                  for (int ks = 0; ks < KS; ++ks) if (ks < ksn) ps = __builtin_amdgcn_mfma_i32_16x16x64_i8(xs[j][ks], wk[ks], ps, 0, 0, 0);
                  const float al = o < g.Opad ? pp.alpha[pidx(g, i, j, k, o)] : 0.f;
                  const float mk = ckl[k * g.nba + j];
#pragma unroll
                  for (int r = 0; r < 4; ++r) {
                    acc[ob][r] += adc_literal_sum(ps, g.mode, sw, sa, al, g.qn, g.qp, mk, r);
                    const bool pass = ste_literal(ps[r], g.mode, sw, sa, al, g.thr_hi, g.thr_lo) != 0.f;
                    const float code = code_literal(ps[r], g.mode, sw, sa, al, g.qn, g.qp, g.thr_hi, g.thr_lo);
                    stw[r] |= st_bits(pass, code) << (3 * j);
                  }
                }
              }
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                if (CST == 4 && k >= 2) stc2[CST == 4 ? ob : 0][r] |= stw[r] << (12 * (k - 2));
                else stc[ob][r] |= stw[r] << (3 * g.nba * k);
              }
            }
          }
        }
      }
      {
        // [T][M][O]: the lane's four pixels of channel o, the 16 lanes of a row on 16 consecutive words
#pragma unroll
        for (int ob = 0; ob < OBM; ++ob) {
          const int o = (og * OBM + ob) * 16 + r16;
          if (ob < nob && o < g.O) {
            const size_t e0 = ((size_t)i * g.M + (size_t)mt * 64 + wave * 16 + 4 * g4) * g.O + o;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              if constexpr (CST == 4)
                reinterpret_cast<uint2*>(st)[e0 + (size_t)r * g.O] = make_uint2(stc[ob][r], stc2[CST == 4 ? ob : 0][r]);
              else
                reinterpret_cast<uint32_t*>(st)[e0 + (size_t)r * g.O] = stc[ob][r];
            }
          }
        }
      }
    }
    // store out (NCHW).  acc[ob][r]: pixel wave*16 + 4*g4 + r, channel (og*OBM + ob)*16 + r16
#pragma unroll
    for (int ob = 0; ob < OBM; ++ob) {
      const int o = (og * OBM + ob) * 16 + r16;
      if (ob < nob && o < g.O) {
        const int m4 = mt * 64 + wave * 16 + 4 * g4;  // M < 2^24 (wide_plan)
        const int bb = fdiv(m4, g.P, inv_p), pq = m4 - bb * g.P;
        const size_t oi = ((size_t)bb * g.O + o) * g.P + pq;
        *reinterpret_cast<float4*>(out + oi) = make_float4(acc[ob][0], acc[ob][1], acc[ob][2], acc[ob][3]);
      }
    }
  }
}

}  // namespace cimq
