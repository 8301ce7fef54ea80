// cimq_kernels_bwd.hip -- the general backward kernels of the CiM conv (any geometry, every ADC variant):
// grad_x as the unfolded product and its fold, grad_w / grad_alpha slabs and the alpha_cim init sums.
#include "cimq_general.h"

namespace cimq {

// =========================================================================================
// cim_bwd_gx: grad wrt the activation   (lsq.py:338-382, closed form)
// =========================================================================================
//   gx_unf[m,f] = sum_{k,o} g[m,o] * E_k[m,i(f),o] * w^_k[f,o]
//   E_k = sum_j 2^-(bsa*j) * mask[k,j] * STE[m,i,k,j,o]
// ps is recomputed TRANSPOSED (rows kappa=(k,o), columns = pixels) so each accumulator is
// directly the B operand of the next bf16 MFMA (contraction over kappa, no LDS transpose);
// g*E is split into three bf16 terms.  Block = (64 pixels, crossbar tile blockIdx.y): the
// tiles' f ranges are disjoint, so every unfolded value gxu[m][f] is written by exactly one
// lane; fold_gx_kernel then applies the nn.Fold adjoint (lsq.py:382) in a fixed order -- no
// atomics anywhere, bit-identical run to run.
template <int NBP, int FBMAX>
__global__ __launch_bounds__(256) void cim_bwd_gx_kernel(Geo g, const int8_t* __restrict__ xcode,
                                                         const v4i* __restrict__ wfrag,
                                                         const v4i* __restrict__ wgx, Params pp,
                                                         const float* __restrict__ sw_p,
                                                         const float* __restrict__ sa_p,
                                                         const float* __restrict__ gout,
                                                         float* __restrict__ gxu) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  TileSmem sm;
  sm.As = reinterpret_cast<int8_t*>(smem);
  size_t off = (size_t)g.nba * 64 * g.KTP;
  sm.foff = reinterpret_cast<int*>(smem + off); off += sizeof(int) * g.KS * 64;
  sm.fkk = reinterpret_cast<int*>(smem + off); off += sizeof(int) * g.KS * 64;
  sm.rowinfo = reinterpret_cast<int4*>(smem + off);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, g4 = lane >> 4;
  const float sw = *sw_p, sa = *sa_p;
  const bool literal = (pp.flags[0] != 0) || g.variant != VAR_LIBRARY;
  const int nkj = g.nbw * g.nba;
  const int m0 = blockIdx.x * 64;
  const int i = blockIdx.y;
  const int flo = i * g.xbar, flen = min(g.xbar, g.K - flo);

  build_rowinfo(g, m0, sm.rowinfo);
  build_ftable(g, i, sm.foff, sm.fkk);
  __syncthreads();
  build_As<NBP>(g, xcode, sm);
  __syncthreads();

  const int mcol = m0 + wave * 16 + r16;  // this lane's pixel (accumulator column)
  const bool mvalid = sm.rowinfo[wave * 16 + r16].w != 0;
  v4f gxa[FBMAX];
#pragma unroll
  for (int fb = 0; fb < FBMAX; ++fb) gxa[fb] = v4f{0.f, 0.f, 0.f, 0.f};

  for (int kc = 0; kc < g.NBLK; kc += 8) {  // chunk of 8 kappa-blocks (4 MFMA K-steps)
    float E[8][4];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) E[a][b] = 0.f;
    for (int j = 0; j < g.nba; ++j) {
      v4i xb[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        if (ks < g.KS) xb[ks] = load_xfrag(g, sm.As, j, wave * 16 + r16, ks, lane);
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        const int kb = kc + kk;
        if (kb < g.NBLK) {
          v4i acc = {0, 0, 0, 0};
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
            if (ks < g.KS)
              acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(
                  wfrag[((size_t)(i * g.KS + ks) * g.NBLK + kb) * WAVE + lane], xb[ks], acc, 0, 0, 0);
          const int k = kb / g.OB16;
          const int obase = (kb - k * g.OB16) * 16 + 4 * g4;
          const float ce = pp.ckj[nkj + k * g.nba + j];
          const int pi = pidx(g, i, j, k, obase);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            bool pass;
            if (!literal) {
              pass = (unsigned)(acc[r] - pp.mlo[pi + r]) <= (unsigned)pp.mhi[pi + r];
            } else {
              const float b = psb_value(g, acc[r], sw, sa, pp.alpha[pi + r], pp.beta[pi + r]);
              pass = ste_pass(b, g.thr_hi, g.thr_lo);
            }
            E[kk][r] += pass ? ce : 0.f;
          }
        }
      }
    }
    // B operands: (g * E)[kappa, pixel], kappa-step s covers kappa-blocks kc+2s, kc+2s+1
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int kb0 = kc + 2 * s;
      if (kb0 < g.NBLK) {
        uint32_t hi[4] = {0, 0, 0, 0}, mi[4] = {0, 0, 0, 0}, lo[4] = {0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int kb = kb0 + (e >> 2);
          const int r = e & 3;
          float av = 0.f;
          if (kb < g.NBLK && mvalid) {
            const int k = kb / g.OB16;
            const int o = (kb - k * g.OB16) * 16 + 4 * g4 + r;
            if (o < g.O) av = gout[(size_t)mcol * g.O + o] * E[2 * s + (e >> 2)][r];
          }
          uint16_t h, md, l;
          split3(av, h, md, l);
          hi[e >> 1] |= (uint32_t)h << (16 * (e & 1));
          mi[e >> 1] |= (uint32_t)md << (16 * (e & 1));
          lo[e >> 1] |= (uint32_t)l << (16 * (e & 1));
        }
        const v8bf bh = as_v8bf(v4i{(int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]});
        const v8bf bm = as_v8bf(v4i{(int)mi[0], (int)mi[1], (int)mi[2], (int)mi[3]});
        const v8bf bl = as_v8bf(v4i{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3]});
        const int sg = kc / 2 + s;
#pragma unroll
        for (int fb = 0; fb < FBMAX; ++fb) {
          if (fb < g.FBT) {
            const v8bf wa = as_v8bf(wgx[((size_t)(i * g.FBT + fb) * g.NKS + sg) * WAVE + lane]);
            gxa[fb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa, bh, gxa[fb], 0, 0, 0);
            gxa[fb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa, bm, gxa[fb], 0, 0, 0);
            gxa[fb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa, bl, gxa[fb], 0, 0, 0);
          }
        }
      }
    }
  }
  // gx_unf[pixel, f] of this tile's rows (accumulator row fb*16 + 4*g4 + r, column = pixel)
  if (mvalid) {
    float* dst = gxu + (size_t)mcol * g.K + flo;
#pragma unroll
    for (int fb = 0; fb < FBMAX; ++fb) {
      if (fb < g.FBT) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = fb * 16 + 4 * g4 + r;
          if (t < flen) dst[t] = gxa[fb][r];
        }
      }
    }
  }
}

// nn.Fold adjoint of the unfold (lsq.py:382): every input element sums its (kh, kw) window
// taps of gx_unf in a fixed order, times sw / nba (lsq.py:362-376's slice recombination).
// Dilation is ignored, as by the reference's Unfold of the forward (lsq.py:141).
__global__ void fold_gx_kernel(Geo g, const float* __restrict__ gxu, const float* __restrict__ sw_p,
                               float* __restrict__ gx) {
  const float scale = (*sw_p) / (float)g.nba;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < g.Nin;
       idx += (long long)gridDim.x * blockDim.x) {
    const int iw = (int)(idx % g.W);
    long long r = idx / g.W;
    const int ih = (int)(r % g.H);
    r /= g.H;
    const int c = (int)(r % g.C);
    const int b = (int)(r / g.C);
    float a = 0.f;
    for (int kh = 0; kh < g.KH; ++kh) {
      const int th = ih + g.PH - kh;
      if (th < 0 || th % g.SH != 0) continue;
      const int oh = th / g.SH;
      if (oh >= g.Ho) continue;
      for (int kw = 0; kw < g.KW; ++kw) {
        const int tw = iw + g.PW - kw;
        if (tw < 0 || tw % g.SW != 0) continue;
        const int ow = tw / g.SW;
        if (ow >= g.Wo) continue;
        const size_t m = (size_t)b * g.P + (size_t)oh * g.Wo + ow;
        a += gxu[m * g.K + (size_t)c * g.KHW + kh * g.KW + kw];
      }
    }
    gx[idx] = a * scale;
  }
}

// =========================================================================================
// cim_bwd_gw: grad wrt the weights and alpha_cim; alpha_cim init   (lsq.py:321-369, 35-87)
// =========================================================================================
//   gw[f,o] = (sa/nbw) * sum_j sum_m xhat_j[m,f] * g[m,o] * D_j[m,i(f),o]
//   D_j = sum_k 2^-(bsw*k) * mask[k,j] * STE[m,i,k,j,o]
//   galpha[i,k,j,o] = c * mask[k,j] * sum_m code[m,i,k,j,o] * g[m,o]
// Block = (tile i, 32-channel group, pixel chunk).  ps is recomputed in the natural
// orientation (rows = pixels), so g*D is directly the B operand of a bf16 MFMA that
// contracts over (pixel, a-slice) against the int8 ctx slices xhat_j (lsq.py:290-295).
// INIT mode accumulates sum_m |ps*sw*sa| instead (fp32 partial sums of lsq.py:64).
template <int NBP, int FBMAX, bool INIT>
__global__ __launch_bounds__(256) void cim_bwd_gw_kernel(Geo g, const int8_t* __restrict__ xcode,
                                                         const int8_t* __restrict__ xhat,
                                                         const v4i* __restrict__ wfrag, Params pp,
                                                         const float* __restrict__ sw_p,
                                                         const float* __restrict__ sa_p,
                                                         const float* __restrict__ signed_p,
                                                         const float* __restrict__ gout, int rows_per_chunk,
                                                         float* __restrict__ gw_slab,
                                                         float* __restrict__ ga_slab,
                                                         float* __restrict__ gb_slab) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  TileSmem sm;
  sm.As = reinterpret_cast<int8_t*>(smem);
  size_t off = (size_t)g.nba * 64 * g.KTP;
  sm.foff = reinterpret_cast<int*>(smem + off); off += sizeof(int) * g.KS * 64;
  sm.fkk = reinterpret_cast<int*>(smem + off); off += sizeof(int) * g.KS * 64;
  sm.rowinfo = reinterpret_cast<int4*>(smem + off); off += sizeof(int4) * 64;
  const int tlen = g.KS * 64;
  const int nkj = g.nbw * g.nba;
  constexpr int NOBG = 1;  // 16-channel output blocks per workgroup (LDS: the per-wave sums below)
  const int ncol = 16 * NOBG;
  // [4 waves][nkj][ncol]: sums of code*g (INIT: of |u|), one writer lane per slot and wave, the
  // waves added in a fixed order at the end -- no atomics, bit-identical run to run
  float* qacc = reinterpret_cast<float*>(smem + off);
  off += sizeof(float) * 4 * nkj * ncol;
  // [FBT*16][ncol] block sum of grad_w: built after the pixel loop, in the act-tile region (free by then)
  float* gwacc = reinterpret_cast<float*>(smem);
  float* qbacc = reinterpret_cast<float*>(smem + off);  // [4 waves][nkj][ncol]: sum beta_term*g (shift variants only)
  off += is_shift(g) ? sizeof(float) * 4 * nkj * ncol : 0;
  int8_t* Xb = reinterpret_cast<int8_t*>(smem + off);   // [nba][tlen][64] bwd slices, f-major

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, g4 = lane >> 4;
  const int i = blockIdx.y;
  const int og = blockIdx.z;  // channel group: o-blocks NOBG*og ..
  const int nob = min(NOBG, g.OB16 - og * NOBG);
  const int mc = blockIdx.x;
  const int mbeg = mc * rows_per_chunk, mend = min(mbeg + rows_per_chunk, g.M);
  const float sw = *sw_p, sa = *sa_p;
  const bool literal = (pp.flags[0] != 0) || g.variant != VAR_LIBRARY;
  const bool ternary_fast = (!literal) && g.mode == ADC_TERNARY;
  const bool has_code = has_alpha(g);
  const bool shift = is_shift(g);

  for (int t = threadIdx.x; t < 4 * nkj * ncol; t += blockDim.x) qacc[t] = 0.f;
  if (!INIT && shift)
    for (int t = threadIdx.x; t < 4 * nkj * ncol; t += blockDim.x) qbacc[t] = 0.f;
  v4f gwa[FBMAX][2];
#pragma unroll
  for (int a = 0; a < FBMAX; ++a) { gwa[a][0] = v4f{0, 0, 0, 0}; gwa[a][1] = v4f{0, 0, 0, 0}; }

  build_ftable(g, i, sm.foff, sm.fkk);
  for (int m0 = mbeg; m0 < mend; m0 += 64) {
    __syncthreads();
    build_rowinfo(g, m0, sm.rowinfo);
    if (threadIdx.x < 64 && m0 + (int)threadIdx.x >= mend) sm.rowinfo[threadIdx.x].w = 0;
    __syncthreads();
    build_As<NBP>(g, xcode, sm);
    if (!INIT) {
      // backward act slices of the int8 ctx code (lsq.py:290-295), f-major: Xb[j][t][row]
      for (int it = threadIdx.x; it < tlen * 16; it += blockDim.x) {
        const int t = it >> 4, rq = (it & 15) * 4;
        const int fk = sm.fkk[t];
        uint32_t pl[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int4 ri = sm.rowinfo[rq + e];
          const uint2 c = gather_code<NBP>(g, xhat, ri, sm.foff[t], fk);
#pragma unroll
          for (int j = 0; j < 4; ++j) pl[j] |= ((c.x >> (8 * j)) & 0xFFu) << (8 * e);
          if (NBP == 8) {
#pragma unroll
            for (int j = 0; j < 4; ++j) pl[4 + j] |= ((c.y >> (8 * j)) & 0xFFu) << (8 * e);
          }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (j < g.nba) *reinterpret_cast<uint32_t*>(Xb + ((size_t)j * tlen + t) * 64 + rq) = pl[j];
      }
    }
    __syncthreads();

    const int rowbase = wave * 16 + 4 * g4;  // this lane's 4 accumulator rows (pixels)
#pragma unroll
    for (int ob = 0; ob < 2; ++ob) {
      if (ob < nob) {
        const int ocol = ob * 16 + r16;
        const int o = og * ncol + ocol;
        float gval[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = m0 + rowbase + r;
          gval[r] = (!INIT && o < g.O && sm.rowinfo[rowbase + r].w) ? gout[(size_t)m * g.O + o] : 0.f;
        }
        float D[8][4];
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) D[a][b] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (j < g.nba) {
            v4i xa[4];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
              if (ks < g.KS) xa[ks] = load_xfrag(g, sm.As, j, wave * 16 + r16, ks, lane);
            for (int k = 0; k < g.nbw; ++k) {
              const int nb = k * g.OB16 + og * NOBG + ob;
              v4i acc = {0, 0, 0, 0};
#pragma unroll
              for (int ks = 0; ks < 4; ++ks)
                if (ks < g.KS)
                  acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(
                      xa[ks], wfrag[((size_t)(i * g.KS + ks) * g.NBLK + nb) * WAVE + lane], acc, 0, 0, 0);
              const int pi = pidx(g, i, j, k, o);
              const int kj = k * g.nba + j;
              float qs = 0.f, qb = 0.f;
              if (INIT) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  const float u = ((float)acc[r] * sw) * sa;  // fp32 ps (no fp16 store), lsq.py:64,84
                  qs += fabsf(u);
                }
              } else {
                const float cd = pp.ckj[2 * nkj + kj];
                if (ternary_fast) {
                  const int mlo = pp.mlo[pi], mhi = pp.mhi[pi], thi = pp.thi[pi], tlo = pp.tlo[pi];
#pragma unroll
                  for (int r = 0; r < 4; ++r) {
                    const int p = acc[r];
                    D[j][r] += ((unsigned)(p - mlo) <= (unsigned)mhi) ? cd : 0.f;
                    const float q = (p >= thi) ? 1.f : ((p <= tlo) ? -1.f : 0.f);
                    qs += q * gval[r];
                  }
                } else {
                  const float al = pp.alpha[pi], be = pp.beta[pi];
                  const int mlo = pp.mlo[pi], mhi = pp.mhi[pi];
#pragma unroll
                  for (int r = 0; r < 4; ++r) {
                    const int p = acc[r];
                    const float b = psb_value(g, p, sw, sa, al, be);
                    const bool pass = literal ? ste_pass(b, g.thr_hi, g.thr_lo) : ((unsigned)(p - mlo) <= (unsigned)mhi);
                    D[j][r] += pass ? cd : 0.f;
                    if (has_code) qs += alpha_term(g, b) * gval[r];
                    if (shift) qb += beta_term(g, b) * gval[r];
                  }
                }
              }
              // lanes l, l^16, l^32, l^48 share the column: fold the 16 pixel rows, then LDS
              qs = rows4_sum(qs);
              if (shift) {
                qb = rows4_sum(qb);
              }
              if (g4 == 0 && (INIT || has_code)) {
                qacc[(wave * nkj + kj) * ncol + ocol] += qs;
                if (!INIT && shift) qbacc[(wave * nkj + kj) * ncol + ocol] += qb;
              }
            }
          }
        }
        if (!INIT) {
          // gw MFMA: contraction over kappa = (pixel row r of this lane's 4, a-slice j)
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            if (2 * s < g.nba) {
              uint32_t hi[4] = {0, 0, 0, 0}, mi[4] = {0, 0, 0, 0}, lo[4] = {0, 0, 0, 0};
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                const int j = 2 * s + (e >> 2), r = e & 3;
                const float bv = (j < g.nba) ? gval[r] * D[j][r] : 0.f;
                uint16_t h, md, l;
                split3(bv, h, md, l);
                hi[e >> 1] |= (uint32_t)h << (16 * (e & 1));
                mi[e >> 1] |= (uint32_t)md << (16 * (e & 1));
                lo[e >> 1] |= (uint32_t)l << (16 * (e & 1));
              }
              const v8bf bh = as_v8bf(v4i{(int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]});
              const v8bf bm = as_v8bf(v4i{(int)mi[0], (int)mi[1], (int)mi[2], (int)mi[3]});
              const v8bf bl = as_v8bf(v4i{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3]});
#pragma unroll
              for (int fb = 0; fb < FBMAX; ++fb) {
                if (fb < g.FBT) {
                  const int t = fb * 16 + r16;
                  uint32_t ad[4] = {0, 0, 0, 0};
#pragma unroll
                  for (int h2 = 0; h2 < 2; ++h2) {
                    const int j = 2 * s + h2;
                    uint32_t bytes = 0;
                    if (j < g.nba)
                      bytes = *reinterpret_cast<const uint32_t*>(Xb + ((size_t)j * tlen + t) * 64 + rowbase);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                      const float xv = (float)(int8_t)((bytes >> (8 * r)) & 0xFF);
                      const int e = h2 * 4 + r;
                      ad[e >> 1] |= (uint32_t)bf16_bits(xv) << (16 * (e & 1));
                    }
                  }
                  const v8bf xa8 = as_v8bf(v4i{(int)ad[0], (int)ad[1], (int)ad[2], (int)ad[3]});
                  v4f accw = gwa[fb][ob];
                  accw = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa8, bh, accw, 0, 0, 0);
                  accw = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa8, bm, accw, 0, 0, 0);
                  accw = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa8, bl, accw, 0, 0, 0);
                  gwa[fb][ob] = accw;
                }
              }
            }
          }
        }
      }
    }
  }

  // ---- block reductions -> slabs (deterministic: the waves in a fixed order, no atomics) ----
  if (!INIT) {
    __syncthreads();
    for (int t = threadIdx.x; t < g.FBT * 16 * ncol; t += blockDim.x) gwacc[t] = 0.f;
    for (int w = 0; w < 4; ++w) {
      __syncthreads();
      if (wave == w) {
#pragma unroll
        for (int fb = 0; fb < FBMAX; ++fb)
          if (fb < g.FBT)
#pragma unroll
            for (int ob = 0; ob < 2; ++ob)
              if (ob < nob)
#pragma unroll
                for (int r = 0; r < 4; ++r) gwacc[(fb * 16 + 4 * g4 + r) * ncol + ob * 16 + r16] += gwa[fb][ob][r];
      }
    }
  }
  __syncthreads();
  const int wq = nkj * ncol;
  for (int t = threadIdx.x; t < nkj * ncol; t += blockDim.x) {
    const int q = t / ncol, col = t - q * ncol;
    const int o = og * ncol + col;
    if (o < g.Opad) {
      const int k = q / g.nba, j = q - k * g.nba;
      const float qv = ((qacc[t] + qacc[wq + t]) + qacc[2 * wq + t]) + qacc[3 * wq + t];
      ga_slab[(((size_t)mc * g.T + i) * nkj + (size_t)k * g.nba + j) * g.Opad + o] = qv;
      if (!INIT && shift)
        gb_slab[(((size_t)mc * g.T + i) * nkj + (size_t)k * g.nba + j) * g.Opad + o] =
            ((qbacc[t] + qbacc[wq + t]) + qbacc[2 * wq + t]) + qbacc[3 * wq + t];
    }
  }
  if (INIT) return;
  for (int t = threadIdx.x; t < g.FBT * 16 * ncol; t += blockDim.x) {
    const int fl = t / ncol, col = t - fl * ncol;
    const int o = og * ncol + col;
    if (o < g.Opad) gw_slab[(((size_t)mc * g.T + i) * (g.FBT * 16) + fl) * g.Opad + o] = gwacc[t];
  }
}

}  // namespace cimq
