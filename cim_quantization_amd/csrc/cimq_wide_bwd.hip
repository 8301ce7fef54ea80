// cimq_wide_bwd.hip -- the backward of a wide module layer (wide_plan: C >= 128) from the compact state words its
// training forward leaves under CIMQ_OPT_WIDE_BWD (cim_fwd_wide_state_kernel): cimq_v7.hip's two formulations with
// the dimension that kept those kernels off such layers cut into pieces.
//
//  * cim_bwd_gx_wide_kernel -- cim_bwd_gx_v8_kernel's unfolded product
//      gx_unf[m, f] = sum_(k, o) W_i[f, (k, o)] * G_i[m, (k, o)],   G_i[m, (k, o)] = g[m, o] * E_k(state word)
//    with the INPUT channels chunked: a workgroup owns (image, band of input rows, channel chunk), and its LDS ring of
//    output rows holds the chunk's (c, kh) rows alone (WideB::cch channels: about 80 KB, two workgroups a CU, where
//    v8's whole-C ring of a 128-channel 32-wide layer would be 220 KB).  It walks the crossbar tiles that hold rows of
//    its chunk -- a tile straddling a chunk edge is walked by both neighbours, each taking its own (c, kh) blocks of
//    four, which never straddle since chunk edges are multiples of four channels -- and, per tile, the OUTPUT blocks in
//    groups of OBX: G of one group is built in registers from grad_out and the lane's state words, multiplied into
//    every (c, kh) block, folded along kw by DPP and ADDED into the ring.  The ring rows of a step are cleared first,
//    so tiles sharing a block and successive groups need no first-write bookkeeping; every ring word has one owner
//    lane, whose additions come in program order: no atomics, the same bits every run.  The kh fold, sw / nba and the
//    fused act-LSQ backward are v8's.
//  * cim_bwd_gw_wide_kernel -- cim_bwd_gw_v7_kernel's weight-gradient conv, a workgroup per (pixel chunk, 16-channel
//    input block, group of OBG output blocks): the bf16 activation planes of a 128-pixel stage are staged once and
//    serve the group's output blocks in turn, each with accumulators of its own (v7 stages them once per block:
//    32 times for a 512-channel output).  Stride 1 only, interleaved words only.
#include "cimq_bwd_dev.h"

namespace cimq {

// E_k of one state word pair: the weighted count of slice k's pass bits (cim_bwd_gx_v8_kernel's decode)
template <int NBW, int NBA>
__device__ inline float wb_ek(uint32_t w0, uint32_t w1, int k, bool std_mask, int bsw, const float* cel) {
  constexpr bool X2 = V7WordsOf<NBW, NBA>::fmt == V7W_32X2;
  const uint32_t w = (X2 && k >= 2) ? w1 : w0;
  const int kk = X2 ? (k & 1) : k;
  if (std_mask) return ldexpf((float)__popc(w & pass_mask_k(kk, NBA)), bsw * k);
  float E = 0.f;
#pragma unroll
  for (int j = 0; j < NBA; ++j) E += ((w >> (3 * (kk * NBA + j))) & 1u) ? cel[k * NBA + j] : 0.f;
  return E;
}

template <int NBW, int NBA, int OBX>
__global__ __launch_bounds__(256) void cim_bwd_gx_wide_kernel(Geo g, V7 v, WideB wb, const uint32_t* __restrict__ st,
                                                              const v4i* __restrict__ wcy, Params pp,
                                                              const float* __restrict__ sw_p,
                                                              const float* __restrict__ sa_p,
                                                              const float* __restrict__ gout,
                                                              const float* __restrict__ x, float* __restrict__ gx,
                                                              float* __restrict__ gsa_part) {
  static_assert(OBX % 2 == 0, "a K-step of the wcy operand holds two output blocks of one weight slice");
  constexpr int NKJ = NBW * NBA;
  constexpr int NPR = OBX / 2;      // block pairs of a group
  constexpr int NKSL = NBW * NPR;   // K-steps of a group: (k, pair)
  constexpr bool X2 = V7WordsOf<NBW, NBA>::fmt == V7W_32X2;
  static_assert(V7WordsOf<NBW, NBA>::fmt != V7W_PLANES, "interleaved words only");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int bid = (int)blockIdx.x;
  const int cc = bid % wb.ncc, bb = bid / wb.ncc;
  const int b = bb / v.nbands, band = bb - b * v.nbands;
  const int c0 = cc * wb.cch, c1 = min(g.C, c0 + wb.cch), nc = c1 - c0;
  const int cp0 = c0 * 3, cp1 = c1 * 3;  // the chunk's (c, kh) rows: multiples of 12
  const int r0 = band * v.RB, r1 = min(g.H, r0 + v.RB);
  const int oh_lo = max(0, r0 - 1), oh_hi = min(g.Ho - 1, r1);  // output rows whose windows touch rows [r0, r1)
  const int nsteps = (oh_hi - oh_lo + v.NRS) / v.NRS;
  const int CPQ = wb.cch * 3;  // ring pitch in (c, kh) rows
  const int RE = v.SWD + 2;    // ring entry: input columns -1 .. SWD of a segment
  const int lsw = v.lw < 4 ? v.lw : 4;
  const int rinv = (65536 + v.RSLOT - 1) / v.RSLOT;
  auto ring_row = [&](int r) { return r - ((r * rinv) >> 16) * v.RSLOT; };
  const int rrow = v.NSEG * CPQ * RE;  // floats per ring row
  float* ring = reinterpret_cast<float*>(smem);
  float* cel = ring + (size_t)v.RSLOT * rrow;
  float* red = cel + 64;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, g4 = lane >> 4;
  const float sw = *sw_p, sa = *sa_p;
  const int Wo = 1 << v.lw;
  for (int t = threadIdx.x; t < NKJ; t += blockDim.x) cel[t] = pp.ckj[NKJ + t];
  __syncthreads();
  bool std_mask;  // the plain binary mask: E_k = 2^(bsw k) * popcount (cim_bwd_gx_v8_kernel)
  {
    const int kl = lane < NKJ ? lane / NBA : 0;
    std_mask = __builtin_amdgcn_ballot_w64(lane < NKJ && cel[lane < NKJ ? lane : 0] != ldexpf(1.f, g.bsw * kl)) == 0ull;
  }
  const float scale = sw / (float)NBA;
  const float inv_sa = 1.f / sa;
  // the tiles holding rows of the chunk
  const int i_lo = (c0 * 9) / g.xbar, i_hi = (c1 * 9 - 1) / g.xbar;
  const int ngrp = (g.OB16 + OBX - 1) / OBX;
  float gpart = 0.f;
  int done = r0 - 1;
  for (int step = 0; step < nsteps; ++step) {
    const int oh_s = oh_lo + step * v.NRS, oh_e = min(oh_hi, oh_s + v.NRS - 1);
    const int q = 16 * wave + r16;
    const int oh = oh_s + (q >> v.lw), ow = q & (Wo - 1);
    const bool pv = oh <= oh_e;
    const int pimg = (oh << v.lw) + ow;
    const size_t m = (size_t)b * g.P + pimg;
    const int seg = ow >> lsw, col = ow & (v.SWD - 1);
    float* rr = ring + (size_t)ring_row(oh - oh_lo) * rrow + seg * CPQ * RE;
    // clear the step's ring rows (the previous step's fold is behind the barrier that closed it)
    for (int r = oh_s; r <= oh_e; ++r) {
      float* z = ring + (size_t)ring_row(r - oh_lo) * rrow;
      for (int t = threadIdx.x; t < rrow; t += blockDim.x) z[t] = 0.f;
    }
    __syncthreads();
    for (int i = i_lo; i <= i_hi; ++i) {
      // the tile's blocks of four (c, kh) rows inside the chunk
      const int cpb_t = ((i * g.xbar) / 3) >> 2;
      const int cpb_a = max(cpb_t, cp0 >> 2);
      const int cpb_b = min(((min(g.K, (i + 1) * g.xbar) - 1) / 3) >> 2, (cp1 >> 2) - 1);
      const int ncb = cpb_b - cpb_a + 1;
      for (int og = 0; og < ngrp; ++og) {
        const int ob0 = og * OBX;
        // grad_out and the state words of this lane's pixel, channels 4 g4 .. + 3 of the group's blocks
        float gv[OBX][4];
        uint32_t sv[OBX][4], sv2[X2 ? OBX : 1][4];
#pragma unroll
        for (int ob = 0; ob < OBX; ++ob) {
          const bool ok = pv && ob0 + ob < g.OB16;
          const int o = (ob0 + ob) * 16 + 4 * g4;
#pragma unroll
          for (int r = 0; r < 4; ++r) gv[ob][r] = ok ? gout[((size_t)b * g.O + o + r) * g.P + pimg] : 0.f;
          if constexpr (X2) {
            uint4 sa4 = make_uint4(0u, 0u, 0u, 0u), sb4 = sa4;
            if (ok) {
              const uint4* s8 = reinterpret_cast<const uint4*>(st + 2 * (((size_t)i * g.M + m) * g.O + o));
              sa4 = s8[0];
              sb4 = s8[1];
            }
            sv[ob][0] = sa4.x; sv2[ob][0] = sa4.y; sv[ob][1] = sa4.z; sv2[ob][1] = sa4.w;
            sv[ob][2] = sb4.x; sv2[ob][2] = sb4.y; sv[ob][3] = sb4.z; sv2[ob][3] = sb4.w;
          } else {
            uint4 s4 = make_uint4(0u, 0u, 0u, 0u);
            if (ok) s4 = *reinterpret_cast<const uint4*>(st + ((size_t)i * g.M + m) * g.O + o);
            sv[ob][0] = s4.x; sv[ob][1] = s4.y; sv[ob][2] = s4.z; sv[ob][3] = s4.w;
          }
        }
        // G of the group, K-step (k, pair p): kappa = (k, block ob0 + 2p + (e >> 2), channel 4 g4 + (e & 3)) -- the
        // operand's K-step s = (k * OB16 + ob0 + 2p) / 2 (OB16 is even: wide_bwd_plan)
        v8bf Gh[NKSL], Gm[NKSL], Gl[NKSL];
#pragma unroll
        for (int sl = 0; sl < NKSL; ++sl) {
          const int k = sl / NPR, pr = sl - k * NPR;
          float Gv[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int ob = 2 * pr + (e >> 2), r = e & 3;
            Gv[e] = gv[ob][r] * wb_ek<NBW, NBA>(sv[ob][r], sv2[X2 ? ob : 0][r], k, std_mask, g.bsw, cel);
          }
          split3x8(Gv, Gh[sl], Gm[sl], Gl[sl]);
        }
        const v4i* wt = wcy + ((size_t)i * v.NCPBT + (cpb_a - cpb_t)) * g.NKS * 64 + lane;
        int soff[NKSL];  // the operand's K-step of (k, pair); -1 past the last block
#pragma unroll
        for (int sl = 0; sl < NKSL; ++sl) {
          const int k = sl / NPR, pr = sl - k * NPR;
          soff[sl] = (ob0 + 2 * pr < g.OB16) ? ((k * g.OB16 + ob0 + 2 * pr) >> 1) * 64 : -1;
        }
#pragma unroll 1
        for (int cb = 0; cb < ncb; ++cb) {
          v4i a[NKSL];
#pragma unroll
          for (int sl = 0; sl < NKSL; ++sl) a[sl] = soff[sl] >= 0 ? wt[(size_t)cb * g.NKS * 64 + soff[sl]] : v4i{0, 0, 0, 0};
          v4f acc = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int sl = 0; sl < NKSL; ++sl) {
            const v8bf aw = as_v8bf(a[sl]);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw, Gh[sl], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw, Gm[sl], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw, Gl[sl], acc, 0, 0, 0);
          }
          // acc[kw] = gx_unf[(cp, kw)][this lane's pixel], cp = (cpb_a + cb) * 4 + g4; pixel ow feeds column ow + kw - 1
          float fn = dpp_from_next(acc[0]);  // kw = 0 of pixel ow + 1
          if (col == v.SWD - 1) fn = 0.f;
          float fp = dpp_from_prev(acc[2]);  // kw = 2 of pixel ow - 1
          if (col == 0) fp = 0.f;
          const float y = (acc[1] + fn) + fp;
          const int cp = (cpb_a + cb) * 4 + g4;
          if (pv) {  // (cp0 <= cp < cp1: whole blocks inside the chunk)
            float* e = rr + (cp - cp0) * RE;
            e[col + 1] += y;
            if (col == 0) e[0] += acc[0];
            if (col == v.SWD - 1) e[v.SWD + 1] += acc[2];
          }
        }
      }
    }
    __syncthreads();
    // fold along kh the input rows whose three output rows are in the ring (cim_bwd_gx_v8_kernel's pass, stride 1)
    const int upto = (oh_e == g.Ho - 1) ? g.H - 1 : oh_e - 1;
    const int f0 = max(done + 1, r0), f1 = min(upto, r1 - 1);
    if (f1 >= f0) {
      const int nf = (f1 - f0 + 1) * nc * g.W;
      for (int t = threadIdx.x; t < nf; t += blockDim.x) {
        const int iw = t & (g.W - 1), rest = t >> v.lwin;
        const int rq = rest / nc;
        const int cl = rest - rq * nc, ih = f0 + rq;
        const int sg = iw >> lsw, cw = iw & (v.SWD - 1);
        const size_t gi = (((size_t)b * g.C + c0 + cl) * g.H + ih) * g.W + iw;
        const float xv = x[gi];
        float a = 0.f;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
          const int oo = ih + 1 - kh;
          if (oo >= oh_lo && oo <= oh_e) {
            const float* e = ring + (size_t)ring_row(oo - oh_lo) * rrow + (cl * 3 + kh) * RE;
            a += e[sg * CPQ * RE + cw + 1];
            if (cw == v.SWD - 1 && sg + 1 < v.NSEG) a += e[(sg + 1) * CPQ * RE];
            if (cw == 0 && sg > 0) a += e[(sg - 1) * CPQ * RE + v.SWD + 1];
          }
        }
        const float gqv = a * scale;
        // autograd of round_pass(clamp(x / sa, 0, Qp)) * sa (lsq.py:549), as cim_bwd_gx_v8_kernel
        const float y1 = xv / sa;
        const float clv = clamp_nan(y1, 0.f, g.lsq_qp);
        const float rr2 = rintf(clv);
        const float rp = (rr2 - clv) + clv;
        const bool pass = (y1 >= 0.f) && (y1 <= g.lsq_qp);
        const float gy = pass ? gqv * sa : 0.f;
        gx[gi] = pass ? gqv : 0.f;
        gpart += gqv * rp;
        gpart += -(gy * (y1 * inv_sa));
      }
      done = f1;
    }
    __syncthreads();
  }
  for (int o = 32; o > 0; o >>= 1) gpart += __shfl_xor(gpart, o);
  if (lane == 0) red[wave] = gpart;
  __syncthreads();
  if (threadIdx.x == 0) gsa_part[bid] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---------------------------------------------------------------------------------------
// grad_w + grad_alpha_cim partials.  block = (pixel chunk, (16-channel input block cb, output group)); a chunk is
// nstage stages of 128 output pixels; in a stage wave w owns pixels 32w .. 32w + 31 (one MFMA K-step) and the lane
// holding channel o and 8 consecutive pixels builds g * D_j in registers, as in cim_bwd_gw_v7_kernel.
// ---------------------------------------------------------------------------------------
template <int NBW, int NBA, int OBG>
__global__ __launch_bounds__(256) void cim_bwd_gw_wide_kernel(Geo g, V7 v, const uint32_t* __restrict__ st,
                                                              const uint8_t* __restrict__ xcb, Params pp,
                                                              const float* __restrict__ gout,
                                                              float* __restrict__ gw_slab,
                                                              float* __restrict__ ga_slab) {
  constexpr int NKJ = NBW * NBA;
  constexpr bool X2 = V7WordsOf<NBW, NBA>::fmt == V7W_32X2;
  static_assert(V7WordsOf<NBW, NBA>::fmt != V7W_PLANES, "interleaved words only");
  constexpr int NGR = 9;  // row groups of 16 per 16-channel block (144 rows)
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int chunk = blockIdx.x;
  const int ngo = (g.OB16 + OBG - 1) / OBG;
  const int cb = (int)blockIdx.y / ngo, ogr = (int)blockIdx.y - cb * ngo;
  const int NTL = v.NTL;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, g4 = lane >> 4;
  const int Wo = 1 << v.lw;
  const int KHW = g.KHW;
  const int i_lo = (cb * 16 * KHW) / g.xbar;
  const int i_hi = (min(g.C, cb * 16 + 16) * KHW - 1) / g.xbar;
  const int ntl = i_hi - i_lo + 1;

  const size_t plane = (size_t)v.KWP;  // one (j, kw) plane, bf16 elements (gw_pitches)
  uint8_t* cur = smem;
  __bf16* pl = reinterpret_cast<__bf16*>(cur); { const size_t pb = (size_t)NBA * 3 * plane * 2; cur += a16(pb > 36864 ? pb : (size_t)36864); }
  float* cdl = reinterpret_cast<float*>(cur); cur += 64 * 4;
  float* red = reinterpret_cast<float*>(cur);  // [OBG][4 waves][NTL][NKJ][16] grad_alpha partials
  const int redw = NTL * NKJ * 16;             // one wave's region
  for (int t = threadIdx.x; t < NKJ; t += blockDim.x) cdl[t] = pp.ckj[2 * NKJ + t];
  // the zero pad after the staged rows of each slice's first plane: fragments of rows past C or outside the image
  const int zoff = v.CPITCH - 8;
  if (threadIdx.x < NBA)
    *reinterpret_cast<uint4*>(pl + (size_t)threadIdx.x * 3 * plane + zoff) = make_uint4(0u, 0u, 0u, 0u);
  for (int t = threadIdx.x; t < OBG * 4 * redw; t += blockDim.x) red[t] = 0.f;
  __syncthreads();
  bool std_mask;  // the plain mask: D_j = 2^(bsa j) * popcount(pass bits of slice j)
  {
    const int kl = lane < NKJ ? lane / NBA : 0, jl = lane < NKJ ? lane - kl * NBA : 0;
    std_mask = __builtin_amdgcn_ballot_w64(lane < NKJ && cdl[lane < NKJ ? lane : 0] != ldexpf(1.f, g.bsa * jl)) == 0ull;
  }
  // A rows f = cb*16*KHW + 16*gr + (lane & 15) = (c, kh, kw): plane offset * 4 + kh per lane and group, its tile per group
  int gpk[NGR], gtile[NGR];
#pragma unroll
  for (int gr = 0; gr < NGR; ++gr) {
    const int f0 = cb * 16 * KHW + 16 * gr, f = f0 + r16;
    const int c = f / KHW, tap = f - c * KHW, kh = tap / 3, kw = tap - 3 * kh;
    gpk[gr] = (c < g.C) ? ((kw * v.KWP + (c - cb * 16) * v.CPITCH) << 2) | kh : -1;
    gtile[gr] = (f0 < g.C * KHW) ? f0 / g.xbar : -1;
  }
  v4f acc[OBG][NGR];
#pragma unroll
  for (int a = 0; a < OBG; ++a)
#pragma unroll
    for (int tp = 0; tp < NGR; ++tp) acc[a][tp] = v4f{0.f, 0.f, 0.f, 0.f};

  const int ng8 = Wo >> 3;
  const int nit = v.CPL * v.NSLOT * ng8;  // staging items (<= 2 per thread, wide_bwd_plan)
  auto stage_geom = [&](int stg, int& b0, int& ih_first) {
    const unsigned m0 = (unsigned)(chunk * v.nstage + stg) * 128u;
    b0 = (int)(m0 / (unsigned)g.P);
    const int pim0 = (int)(m0 - (unsigned)b0 * (unsigned)g.P);
    ih_first = v.whole ? 0 : (pim0 >> v.lw) - g.PH;
  };
  int it_cl[2], it_db[2], it_ih[2], it_c8[2];
#pragma unroll
  for (int u2 = 0; u2 < 2; ++u2) {
    const int it = threadIdx.x + u2 * 256;
    const int cl = it / (v.NSLOT * ng8), rem = it - cl * (v.NSLOT * ng8);
    const int slot = rem >> (v.lw - 3), c8 = rem & (ng8 - 1);
    it_cl[u2] = cl;
    it_c8[u2] = c8;
    it_db[u2] = v.whole ? slot / g.H : 0;
    it_ih[u2] = v.whole ? slot - it_db[u2] * g.H : slot;
  }
  const int nstages_all = g.M >> 7;
  for (int stg = 0; stg < v.nstage; ++stg) {
    if (chunk * v.nstage + stg >= nstages_all) break;  // (uniform: the last chunk may hold fewer stages)
    int b0, ih_first;
    stage_geom(stg, b0, ih_first);
    __syncthreads();  // the previous stage's reads of the planes are done
    // bf16 planes of the staged rows: item (channel cl, row slot, 8-column group), the three kw shifts
#pragma unroll
    for (int u2 = 0; u2 < 2; ++u2) {
      const int it = threadIdx.x + u2 * 256;
      if (it < nit) {
        const int cl = it_cl[u2], c8 = it_c8[u2];
        const int bq = b0 + it_db[u2], ih = ih_first + it_ih[u2];
        const int c = cb * 16 + cl;
        uint32_t w[10];
#pragma unroll
        for (int u = 0; u < 10; ++u) w[u] = 0u;
        if (c < g.C && ih >= 0 && ih < g.H && bq < g.B) {
          const uint32_t* src = reinterpret_cast<const uint32_t*>(xcb) + (((size_t)bq * g.C + c) * g.H + ih) * g.W + c8 * 8;
          xload<8>(src, &w[1]);
          if (c8 > 0) w[0] = src[-1];
          if (c8 * 8 + 8 < g.W) w[9] = src[8];
        }
        const int slot = v.whole ? it_db[u2] * g.H + it_ih[u2] : it_ih[u2];
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
#pragma unroll
          for (int j = 0; j < NBA; ++j) {
            uint32_t pk[4];
#pragma unroll
            for (int e2 = 0; e2 < 4; ++e2) {
              const float f0 = (float)(int8_t)xbyte(w[2 * e2 + kw], j);
              const float f1 = (float)(int8_t)xbyte(w[2 * e2 + 1 + kw], j);
              pk[e2] = __builtin_amdgcn_perm(__float_as_uint(f1), __float_as_uint(f0), 0x07060302u);  // exact bf16
            }
            __bf16* dst = pl + (size_t)(j * 3 + kw) * plane + cl * v.CPITCH + slot * Wo + c8 * 8;
            *reinterpret_cast<uint4*>(dst) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
          }
        }
      }
    }
    __syncthreads();
    // this wave's K-step: pixels mk .. mk + 31; this lane's 8 pixels mk8 .. mk8 + 7 (one output row)
    const size_t mk8 = ((size_t)chunk * v.nstage + stg) * 128 + 32 * wave + 8 * g4;
    int b = b0, pimg;
    {
      const int moff = 32 * wave + 8 * g4;
      if (v.whole) {
        const int lp = __builtin_ctz(g.P);
        b = b0 + (moff >> lp);
        pimg = moff & (g.P - 1);
      } else {
        pimg = (int)((unsigned)(chunk * v.nstage + stg) * 128u - (unsigned)b0 * (unsigned)g.P) + moff;
      }
    }
    const int oh = pimg >> v.lw, ow0 = pimg & (Wo - 1);
    int slot_kh[3];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int ih = oh - g.PH + kh;
      int sl = -1;
      if (ih >= 0 && ih < g.H) sl = v.whole ? (b - b0) * g.H + ih : ih - ih_first;
      slot_kh[kh] = sl;
    }
#pragma unroll
    for (int obl = 0; obl < OBG; ++obl) {
      const int ob = ogr * OBG + obl;
      if (ob >= g.OB16) continue;  // (uniform: a partial last group)
      const int o = ob * 16 + r16;
      float gv[8];
      {
        const float4* gp = reinterpret_cast<const float4*>(gout + ((size_t)b * g.O + o) * g.P + pimg);
        const float4 a0 = gp[0], a1 = gp[1];
        gv[0] = a0.x; gv[1] = a0.y; gv[2] = a0.z; gv[3] = a0.w;
        gv[4] = a1.x; gv[5] = a1.y; gv[6] = a1.z; gv[7] = a1.w;
      }
      auto load_state = [&](int i, uint32_t (&sv)[8], uint32_t (&sh)[8]) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if constexpr (X2) {
            const uint2 w = reinterpret_cast<const uint2*>(st)[((size_t)i * g.M + mk8 + e) * g.O + o];
            sv[e] = w.x; sh[e] = w.y;
          } else {
            sv[e] = st[((size_t)i * g.M + mk8 + e) * g.O + o];
            sh[e] = 0u;
          }
        }
      };
      uint32_t sv[8], sh[8];
      load_state(i_lo, sv, sh);
#pragma unroll 1
      for (int tl = 0; tl < ntl; ++tl) {
        const int i = i_lo + tl;
        uint32_t nv[8], nh[8];  // the next tile's words, in flight behind this tile's MFMAs
        if (tl + 1 < ntl) load_state(i + 1, nv, nh);
        // grad_alpha partials (lsq.py:321-333), owned by the block holding the tile's first row: sum of code * g
        if (((i * g.xbar) / KHW) / 16 == cb) {
#pragma unroll
          for (int kj = 0; kj < NKJ; ++kj) {
            float q = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              int code;  // the signed 2-bit field {nz, neg} at bits 3 kj + 1 .. + 2
              if constexpr (X2) code = ((int)((kj < 8 ? sv[e] : sh[e]) << (29 - 3 * (kj & 7)))) >> 30;
              else code = ((int)(sv[e] << (29 - 3 * kj))) >> 30;
              q = __builtin_fmaf((float)code, gv[e], q);
            }
            q = rows4_sum(q);
            if (g4 == 0) red[(obl * 4 + wave) * redw + (tl * NKJ + kj) * 16 + r16] += q;
          }
        }
        // B operands: g * D_j, D_j = sum_k cD_kj * pass_ijk, split into bf16 hi / mid / lo
        v8bf bh[NBA], bm[NBA], bq[NBA];
#pragma unroll
        for (int j = 0; j < NBA; ++j) {
          float d[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            float D;
            if constexpr (X2) {
              if (std_mask) {
                const uint32_t mj = pass_mask_j(j, 2, NBA);
                D = ldexpf((float)__popc((sv[e] & mj) | ((sh[e] & mj) << 1)), g.bsa * j);
              } else {
                D = 0.f;
#pragma unroll
                for (int k = 0; k < NBW; ++k)
                  D += (((k < 2 ? sv[e] : sh[e]) >> (3 * ((k & 1) * NBA + j))) & 1u) ? cdl[k * NBA + j] : 0.f;
              }
            } else if (std_mask) {
              D = ldexpf((float)__popc(sv[e] & pass_mask_j(j, NBW, NBA)), g.bsa * j);
            } else {
              D = 0.f;
#pragma unroll
              for (int k = 0; k < NBW; ++k) D += ((sv[e] >> (3 * (k * NBA + j))) & 1u) ? cdl[k * NBA + j] : 0.f;
            }
            d[e] = gv[e] * D;
          }
          split3x8(d, bh[j], bm[j], bq[j]);
        }
#pragma unroll
        for (int gr = 0; gr < NGR; ++gr) {
          if (gtile[gr] != i) continue;  // uniform: the row groups of tile i
          const int kh = gpk[gr] & 3;
          const int sl = kh == 0 ? slot_kh[0] : (kh == 1 ? slot_kh[1] : slot_kh[2]);
          const bool ok = gpk[gr] >= 0 && sl >= 0;
          const __bf16* src = pl + (ok ? (gpk[gr] >> 2) + sl * Wo + ow0 : zoff);
#pragma unroll
          for (int j = 0; j < NBA; ++j) {
            const v8bf a = as_v8bf(*reinterpret_cast<const v4i*>(src + (size_t)j * 3 * plane));
            acc[obl][gr] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bh[j], acc[obl][gr], 0, 0, 0);
            acc[obl][gr] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bm[j], acc[obl][gr], 0, 0, 0);
            acc[obl][gr] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bq[j], acc[obl][gr], 0, 0, 0);
          }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) { sv[e] = nv[e]; sh[e] = nh[e]; }
      }
    }
  }
  // reduce the four waves' partials through LDS (the planes are free now), one output block at a time, in a fixed
  // order; then the slabs
  float* gred = reinterpret_cast<float*>(pl);  // [4 waves][NGR][16 rows f][16 o]
  const int FR = g.FBT * 16;
#pragma unroll
  for (int obl = 0; obl < OBG; ++obl) {
    const int ob = ogr * OBG + obl;
    if (ob >= g.OB16) continue;  // (uniform)
    __syncthreads();
#pragma unroll
    for (int gr = 0; gr < NGR; ++gr)
#pragma unroll
      for (int r = 0; r < 4; ++r) gred[((wave * NGR + gr) * 16 + 4 * g4 + r) * 16 + r16] = acc[obl][gr][r];
    __syncthreads();
    for (int t = threadIdx.x; t < NGR * 256; t += blockDim.x) {
      const int oc = t & 15;
      const int f = cb * 16 * KHW + (t >> 4);
      if (f < g.C * KHW) {
        const int i = f / g.xbar, fl = f - i * g.xbar;
        const float sum = (gred[t] + gred[NGR * 256 + t]) + (gred[2 * NGR * 256 + t] + gred[3 * NGR * 256 + t]);
        gw_slab[(((size_t)chunk * g.T + i) * FR + fl) * g.Opad + ob * 16 + oc] = sum;
      }
    }
    for (int t = threadIdx.x; t < ntl * NKJ * 16; t += blockDim.x) {
      const int tl = t / (NKJ * 16), rem = t - tl * NKJ * 16, kj = rem >> 4, oc = rem & 15;
      const int i = i_lo + tl;
      if (((i * g.xbar) / KHW) / 16 == cb) {
        const float* rq = red + (size_t)obl * 4 * redw;
        const float sum = (rq[t] + rq[redw + t]) + (rq[2 * redw + t] + rq[3 * redw + t]);
        ga_slab[(((size_t)chunk * g.T + i) * NKJ + kj) * g.Opad + ob * 16 + oc] = sum;
      }
    }
  }
}

}  // namespace cimq
