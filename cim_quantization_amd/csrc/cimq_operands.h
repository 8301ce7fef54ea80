// cimq_operands.h -- how the kernels' operands are made from x, w and alpha: the activation slice words
// (forward slices and backward ctx slices of one element), the bit slices of a weight and every MFMA weight
// operand layout built from them, and the ADC thresholds / STE intervals.  Used by the prologue kernels
// (cimq_prep.hip, cimq_lsq.hip), the per-family prep kernels, and the kernels that quantise while staging.
#pragma once
#include "cimq_device.h"

namespace cimq {

// =========================================================================================
// prep_act: per input element, the forward bit-slice integers and the backward ctx slices
// =========================================================================================
// x_int = x_q / sa (lsq.py:97); with RAW_LSQ, x_q = round_pass(clamp(x/sa,0,Qp))*sa first
// (lsq.py:549).  Forward slices follow slicing_act / slicing_act_signed on x_int
// (lsq.py:146-149) and are stored as rint() int8s (|residue| << 0.5, so the int8 MAC gives
// round(ps_ref)).  Backward slices are those of the int8 ctx code int8(x_int) (lsq.py:99,
// truncation + wrap) as re-sliced by the backward (lsq.py:290-295).  Both are written as
// NBP-byte words per element (byte j = slice j), once, so no kernel re-slices per gather.
__device__ inline void pack_word(int8_t (&v)[8], int nbp, uint8_t* dst, long long idx) {
  uint32_t lo = (uint8_t)v[0] | ((uint32_t)(uint8_t)v[1] << 8) | ((uint32_t)(uint8_t)v[2] << 16) |
                ((uint32_t)(uint8_t)v[3] << 24);
  if (nbp == 4) {
    reinterpret_cast<uint32_t*>(dst)[idx] = lo;
  } else {
    uint2 w;
    w.x = lo;
    w.y = (uint8_t)v[4] | ((uint32_t)(uint8_t)v[5] << 8) | ((uint32_t)(uint8_t)v[6] << 16) |
          ((uint32_t)(uint8_t)v[7] << 24);
    reinterpret_cast<uint2*>(dst)[idx] = w;
  }
}

// WB (here and in the helpers below): also write the backward (ctx) words to xcb; false for the forward-only
// prologues (CIMQ_OPT_INFERENCE), whose ctx has no such region
template <bool WB = true>
__device__ inline void act_item(const Geo& g, const float* __restrict__ x, float sa, bool sgn,
                                uint8_t* __restrict__ xcf, uint8_t* __restrict__ xcb, long long idx) {
  float v = x[idx];
  float xq;
  if (g.input_kind == 1) {
    float t = v / sa;
    float c = clamp_nan(t, 0.f, g.lsq_qp);
    float r = rintf(c);
    float rp = (r - c) + c;  // round_pass value
    xq = rp * sa;
  } else {
    xq = v;
  }
  const float xi = xq / sa;
  const float xh = (float)to_i8_wrap(xi);
  int8_t fw[8], bw[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float s = 0.f, sb = 0.f;
    if (j < g.nba) {
      s = sgn ? slice_signed(xi, j, g.bsa) : slice_unsigned(xi, j, g.bsa);
      sb = sgn ? slice_signed(xh, j, g.bsa) : slice_unsigned(xh, j, g.bsa);
    }
    fw[j] = (j < g.nba) ? (int8_t)clamp_i8(s) : (int8_t)0;
    bw[j] = (j < g.nba) ? (int8_t)clamp_i8(sb) : (int8_t)0;
  }
  pack_word(fw, g.NBP, xcf, idx);
  if constexpr (WB) pack_word(bw, g.NBP, xcb, idx);
}

// Slice words of one element, NBP-specialised.  When x_int is an exact integer (the common
// case: fl(fl(r*sa)/sa) == r) the floor / remainder chain of slicing_act(_signed) reduces to
// shifts and masks of that integer, bit for bit (floor-mod by 2^b of an integer is its low b
// bits in two's complement); other values (the 6 - eps slice artifacts) take the float path.
// NBA_C > 0: nba = NBA_C and bsa = 1 at compile time (the unrolled digit loop has no runtime
// bounds); 0: read from g
template <int NBP, int NBA_C = 0>
__device__ inline void act_words_xq(const Geo& g, float xq, float sa, bool sgn, uint32_t (&fwd)[NBP / 4],
                                    uint32_t (&bwd)[NBP / 4]) {
  const int nba = NBA_C > 0 ? NBA_C : g.nba;
  const int bsa = NBA_C > 0 ? 1 : g.bsa;
  const float xi = xq / sa;
  const int xhi = to_i8_wrap(xi);
  const int mask = (1 << bsa) - 1;
  // forward digits without branches for |xi| < 2^23: with F = floor(m) and fr = m - F (both
  // exact), m = xi (unsigned) or |xi| (signed, digits negated for xi < 0), the reference's
  // chain gives digit 0 = rint((F mod 2^b) + fr) -- 2^b for the 6 - eps artifacts -- and digit
  // j = (F >> b*j) mod 2^b (floor(floor(m) / 2^s) = floor(m / 2^s)); larger |xi| or NaN take
  // the float chain below
  const bool fast = fabsf(xi) < 8388608.f;
  const float m = sgn ? fabsf(xi) : xi;
  const float F = floorf(m);
  const int Fi = fast ? (int)F : 0;
  const float fr = m - F;
  const bool negd = sgn && xi < 0.f;
#pragma unroll
  for (int w = 0; w < NBP / 4; ++w) { fwd[w] = 0u; bwd[w] = 0u; }
#pragma unroll
  for (int j = 0; j < NBP; ++j) {
    if (j < nba) {
      const int sh = bsa * j;
      const int sb = sgn ? (xhi >= 0 ? ((xhi >> sh) & mask) : -(((-xhi) >> sh) & mask)) : ((xhi >> sh) & mask);
      int d = (j == 0) ? min((int)rintf((float)(Fi & mask) + fr), 127) : ((Fi >> sh) & mask);
      const int sf = negd ? -d : d;
      fwd[j >> 2] |= (uint32_t)(uint8_t)(int8_t)sf << (8 * (j & 3));
      bwd[j >> 2] |= (uint32_t)(uint8_t)(int8_t)sb << (8 * (j & 3));
    }
  }
  if (!fast) {
#pragma unroll
    for (int w = 0; w < NBP / 4; ++w) fwd[w] = 0u;
#pragma unroll
    for (int j = 0; j < NBP; ++j) {
      if (j < nba) {
        const int sf = clamp_i8(sgn ? slice_signed(xi, j, bsa) : slice_unsigned(xi, j, bsa));
        fwd[j >> 2] |= (uint32_t)(uint8_t)(int8_t)sf << (8 * (j & 3));
      }
    }
  }
}

// x_q of one element: with RAW_LSQ the activation quantiser round_pass(clamp(x/sa,0,Qp))*sa
// (lsq.py:549), else the input itself
__device__ inline float act_xq(const Geo& g, float v, float sa) {
  if (g.input_kind != 1) return v;
  const float t = v / sa;
  const float c = clamp_nan(t, 0.f, g.lsq_qp);
  const float r = rintf(c);
  const float rp = (r - c) + c;  // round_pass value
  return rp * sa;
}

template <int NBP, int NBA_C = 0>
__device__ inline void act_words(const Geo& g, float v, float sa, bool sgn, uint32_t (&fwd)[NBP / 4],
                                 uint32_t (&bwd)[NBP / 4]) {
  act_words_xq<NBP, NBA_C>(g, act_xq(g, v, sa), sa, sgn, fwd, bwd);
}

// RAW_LSQ: the words depend on the element only through the integer code r = rint(clamp(x/sa,
// 0, Qp)) -- round_pass gives rp = (r - c) + c = r exactly for c in [0, Qp], so x_q = r * sa --
// so a block tabulates the Qp + 1 words once (with the same act_words_xq) and each element
// takes the quantiser's division, clamp and rint, then a table lookup; a NaN code (NaN input)
// takes the element-wise chain.  lut: [Qp + 1][fwd words, bwd words] in LDS.
template <int NBP, int NBA_C>
__device__ inline void act_lut_build(const Geo& g, float sa, bool sgn, uint32_t* lut) {
  const int nl = (int)g.lsq_qp + 1;
  for (int r = threadIdx.x; r < nl; r += blockDim.x) {
    uint32_t f[NBP / 4], b[NBP / 4];
    act_words_xq<NBP, NBA_C>(g, (float)r * sa, sa, sgn, f, b);
#pragma unroll
    for (int w = 0; w < NBP / 4; ++w) {
      lut[r * (NBP / 2) + w] = f[w];
      lut[r * (NBP / 2) + NBP / 4 + w] = b[w];
    }
  }
  __syncthreads();
}
template <int NBP, int NBA_C>
__device__ inline void act_words_lut(const Geo& g, float v, float sa, bool sgn, const uint32_t* lut,
                                     uint32_t (&fwd)[NBP / 4], uint32_t (&bwd)[NBP / 4]) {
  const float c = clamp_nan(v / sa, 0.f, g.lsq_qp);
  const float r = rintf(c);
  if (r == r) {
    const int e = (int)r * (NBP / 2);
    if (NBP == 4) {
      const uint2 t = *reinterpret_cast<const uint2*>(lut + e);
      fwd[0] = t.x;
      bwd[0] = t.y;
    } else {
      const uint4 t = *reinterpret_cast<const uint4*>(lut + e);
      fwd[0] = t.x;
      fwd[NBP / 4 - 1] = t.y;
      bwd[0] = t.z;
      bwd[NBP / 4 - 1] = t.w;
    }
  } else {
    act_words<NBP, NBA_C>(g, v, sa, sgn, fwd, bwd);
  }
}

// four consecutive elements (idx4 = 4 * t): one 16-B load, 16-B (NBP 4) or 2 x 16-B stores
template <int NBP, int NBA_C = 0, bool WB = true>
__device__ inline void act_item4(const Geo& g, const float* __restrict__ x, float sa, bool sgn,
                                 uint8_t* __restrict__ xcf, uint8_t* __restrict__ xcb, long long t,
                                 const uint32_t* lut = nullptr) {
  const float4 v4 = reinterpret_cast<const float4*>(x)[t];
  const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
  uint32_t f[4][NBP / 4], b[4][NBP / 4];
  if (lut) {
#pragma unroll
    for (int e = 0; e < 4; ++e) act_words_lut<NBP, NBA_C>(g, vv[e], sa, sgn, lut, f[e], b[e]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) act_words<NBP, NBA_C>(g, vv[e], sa, sgn, f[e], b[e]);
  }
  if (NBP == 4) {
    reinterpret_cast<uint4*>(xcf)[t] = make_uint4(f[0][0], f[1][0], f[2][0], f[3][0]);
    if constexpr (WB) reinterpret_cast<uint4*>(xcb)[t] = make_uint4(b[0][0], b[1][0], b[2][0], b[3][0]);
  } else {
    reinterpret_cast<uint4*>(xcf)[2 * t] = make_uint4(f[0][0], f[0][NBP / 4 - 1], f[1][0], f[1][NBP / 4 - 1]);
    reinterpret_cast<uint4*>(xcf)[2 * t + 1] = make_uint4(f[2][0], f[2][NBP / 4 - 1], f[3][0], f[3][NBP / 4 - 1]);
    if constexpr (WB) {
      reinterpret_cast<uint4*>(xcb)[2 * t] = make_uint4(b[0][0], b[0][NBP / 4 - 1], b[1][0], b[1][NBP / 4 - 1]);
      reinterpret_cast<uint4*>(xcb)[2 * t + 1] = make_uint4(b[2][0], b[2][NBP / 4 - 1], b[3][0], b[3][NBP / 4 - 1]);
    }
  }
}

// all elements of x: vectorised when Nin % 4 == 0 (W % 4 == 0), element-wise otherwise
template <int NBP, int NBA_C, bool WB = true>
__device__ inline void act_range_sel(const Geo& g, const float* __restrict__ x, float sa, bool sgn,
                                     uint8_t* __restrict__ xcf, uint8_t* __restrict__ xcb, long long first,
                                     long long step, uint32_t* lut) {
  const long long n4 = g.Nin / 4;
  const bool tab = lut && g.input_kind == 1 && g.lsq_qp >= 0.f && g.lsq_qp < (float)kActLutMax;
  if (tab) act_lut_build<NBP, NBA_C>(g, sa, sgn, lut);  // block-uniform condition: every thread syncs
  for (long long t = first; t < n4; t += step) act_item4<NBP, NBA_C, WB>(g, x, sa, sgn, xcf, xcb, t, tab ? lut : nullptr);
}

// lut: LDS for the RAW_LSQ word table (kActLutMax * NBP / 2 words), or null; called by every
// thread of the block
template <bool WB = true>
__device__ inline void act_range(const Geo& g, const float* __restrict__ x, float sa, bool sgn,
                                 uint8_t* __restrict__ xcf, uint8_t* __restrict__ xcb, long long first,
                                 long long step, uint32_t* lut = nullptr) {
  if (g.Nin % 4 == 0) {
    const long long n4 = g.Nin / 4;
    // the 1-bit-slice cases of the CIFAR / QuantLinear configs with compile-time digit loops
    const int sel = g.bsa != 1 ? 0 : g.nba;
    if (sel == 3)
      act_range_sel<4, 3, WB>(g, x, sa, sgn, xcf, xcb, first, step, lut);
    else if (sel == 2)
      act_range_sel<4, 2, WB>(g, x, sa, sgn, xcf, xcb, first, step, lut);
    else if (sel == 4)
      act_range_sel<4, 4, WB>(g, x, sa, sgn, xcf, xcb, first, step, lut);
    else if (sel == 8)
      act_range_sel<8, 8, WB>(g, x, sa, sgn, xcf, xcb, first, step, lut);
    else if (g.NBP == 4)
      for (long long t = first; t < n4; t += step) act_item4<4, 0, WB>(g, x, sa, sgn, xcf, xcb, t);
    else
      for (long long t = first; t < n4; t += step) act_item4<8, 0, WB>(g, x, sa, sgn, xcf, xcb, t);
  } else {
    for (long long idx = first; idx < g.Nin; idx += step) act_item<WB>(g, x, sa, sgn, xcf, xcb, idx);
  }
}

// act_range for an input that arrives as activation codes (cimq_module_forward_codes: forward words only): the
// element's words are the table entry of its byte -- entries 0 .. Qp as act_lut_build makes them, entry Qp + 1 the
// words of a NaN element (act_words of any NaN: its chain is independent of the NaN's sign and payload); a byte
// above Qp + 1 reads that entry too, so none indexes past the table.  lut: (Qp + 2) * NBP / 2 words of LDS
// (Qp <= 254: within kActLutMax entries); called by every thread of the block.
template <int NBP>
__device__ inline void act_range_codes(const Geo& g, const uint8_t* __restrict__ xq, float sa, bool sgn,
                                       uint8_t* __restrict__ xcf, long long first, long long step, uint32_t* lut) {
  constexpr int NW = NBP / 4;
  const int nan_e = (int)g.lsq_qp + 1;
  if (threadIdx.x == 0) {
    uint32_t f[NW], b[NW];
    act_words<NBP, 0>(g, __int_as_float(0x7fc00000), sa, sgn, f, b);
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      lut[nan_e * (NBP / 2) + w] = f[w];
      lut[nan_e * (NBP / 2) + NW + w] = b[w];
    }
  }
  act_lut_build<NBP, 0>(g, sa, sgn, lut);  // entries 0 .. Qp, then the block barrier
  uint32_t* dst = reinterpret_cast<uint32_t*>(xcf);
  if (g.Nin % 4 == 0) {
    const long long n4 = g.Nin / 4;
    for (long long t = first; t < n4; t += step) {
      const uint32_t cw = reinterpret_cast<const uint32_t*>(xq)[t];
      uint32_t f[4][NW];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = min((int)((cw >> (8 * e)) & 255u), nan_e) * (NBP / 2);
#pragma unroll
        for (int w = 0; w < NW; ++w) f[e][w] = lut[c + w];
      }
      if (NBP == 4) {
        reinterpret_cast<uint4*>(xcf)[t] = make_uint4(f[0][0], f[1][0], f[2][0], f[3][0]);
      } else {
        reinterpret_cast<uint4*>(xcf)[2 * t] = make_uint4(f[0][0], f[0][NW - 1], f[1][0], f[1][NW - 1]);
        reinterpret_cast<uint4*>(xcf)[2 * t + 1] = make_uint4(f[2][0], f[2][NW - 1], f[3][0], f[3][NW - 1]);
      }
    }
  } else {
    for (long long idx = first; idx < g.Nin; idx += step) {
      const int c = min((int)xq[idx], nan_e) * (NBP / 2);
#pragma unroll
      for (int w = 0; w < NW; ++w) dst[idx * NW + w] = lut[c + w];
    }
  }
}

// =========================================================================================
// prep_weight: MFMA fragments of the weight bit slices
// =========================================================================================
// w_int = w_q / sw (lsq.py:98), w_unf = w_int.view(O,-1).t() (lsq.py:153), signed slices
// (lsq.py:155).  Forward / ps-recompute operand: rint(slice) as int8, stored in the exact
// per-lane order of v_mfma_i32_16x16x64_i8: wfrag[i][ks][nb][lane][16 bytes], lane l holding
// rows n = nb*16 + (l&15) (n = k*Opad + o) and contraction f = i*xbar + ks*64 + 16*(l>>4) + e.
// grad_x operand: int8(slice) (lsq.py:160 truncation) as bf16, wgx[i][fb][s][lane][8]:
// lane l holds f = i*xbar + fb*16 + (l&15), kappa = (2s + (e>>2))*16 + 4*(l>>4) + (e&3).
// Source of the integer weights w_int = w_q / sw: either a materialised w_q (Function entry
// points) or the raw weight run through the LSQ quantiser in place (module entry points:
// w_q = round_pass(clamp(w / sw, Qn, Qp)) * sw, lsq.py:555, the same fp32 op sequence).
struct WSrc {
  const float* w;
  float sw;
  int raw;
  float qn, qp;
  __device__ float wint(const Geo& g, int o, int f) const {
    const float v = w[(size_t)o * g.K + f];
    if (!raw) return v / sw;
    const float c = clamp_nan(v / sw, qn, qp);
    const float wq = round_pass_value(c) * sw;
    return wq / sw;
  }
};

__device__ inline float wslice(const Geo& g, const WSrc& ws, int f, int n) {
  const int k = n / g.Opad, o = n - k * g.Opad;
  if (f >= g.K || o >= g.O || k >= g.nbw) return 0.f;
  return slice_signed(ws.wint(g, o, f), k, g.bsw);
}

__device__ inline void wfrag_item(const Geo& g, const WSrc& ws, v4i* __restrict__ wfrag, int t) {
  const int lane = t % WAVE;
  int r = t / WAVE;
  const int nb = r % g.NBLK;
  r /= g.NBLK;
  const int ks = r % g.KS;
  const int i = r / g.KS;
  const int flo = i * g.xbar, fhi = min(flo + g.xbar, g.K);
  const int n = nb * 16 + (lane & 15);
  uint32_t wd[4] = {0, 0, 0, 0};
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int f = flo + ks * 64 + 16 * (lane >> 4) + e;
    int v = 0;
    if (f < fhi) v = clamp_i8(wslice(g, ws, f, n));
    wd[e >> 2] |= ((uint32_t)(uint8_t)(int8_t)v) << (8 * (e & 3));
  }
  v4i o;
  o.x = (int)wd[0]; o.y = (int)wd[1]; o.z = (int)wd[2]; o.w = (int)wd[3];
  wfrag[t] = o;
}

__device__ inline void wgx_item(const Geo& g, const WSrc& ws, v4i* __restrict__ wgx, int t) {
  const int lane = t % WAVE;
  int r = t / WAVE;
  const int s = r % g.NKS;
  r /= g.NKS;
  const int fb = r % g.FBT;
  const int i = r / g.FBT;
  const int flo = i * g.xbar, fhi = min(flo + g.xbar, g.K);
  const int f = flo + fb * 16 + (lane & 15);
  uint32_t wd[4] = {0, 0, 0, 0};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int kb = 2 * s + (e >> 2);
    const int kap = kb * 16 + 4 * (lane >> 4) + (e & 3);
    float v = 0.f;
    if (f < fhi && kb < g.NBLK) v = (float)to_i8_wrap(wslice(g, ws, f, kap));
    const uint32_t h = bf16_bits(v);
    wd[e >> 1] |= h << (16 * (e & 1));
  }
  v4i o;
  o.x = (int)wd[0]; o.y = (int)wd[1]; o.z = (int)wd[2]; o.w = (int)wd[3];
  wgx[t] = o;
}

// v8 grad_x operand (cimq_v7.hip): the same int8(slice) values as wgx with the MFMA rows
// re-ordered so that row rho = 4*q + kw of cp-block cpb is weight row f = cp*KW + kw,
// cp = cpb*4 + q = c*KH + kh (rho & 3 == 3 and rows outside tile i are zero): one lane of the
// product then holds all KW taps of one (c, kh) for its pixel.  wcy[i][cb][s][lane][8 bf16],
// cpb = cpb_lo(i) + cb, cpb_lo(i) = ((i*xbar) / KW) / 4, cb < ncpbt.
__device__ inline void wcy_item(const Geo& g, const WSrc& ws, int ncpbt, v4i* __restrict__ wcy, int t) {
  const int lane = t % WAVE;
  int r = t / WAVE;
  const int s = r % g.NKS;
  r /= g.NKS;
  const int cb = r % ncpbt;
  const int i = r / ncpbt;
  const int flo = i * g.xbar, fhi = min(flo + g.xbar, g.K);
  const int rho = lane & 15;
  const int cp = ((flo / g.KW) / 4 + cb) * 4 + (rho >> 2), kw = rho & 3;
  const int c = cp / g.KH, kh = cp - c * g.KH;
  const int f = c * g.KHW + kh * g.KW + kw;
  const bool ok = kw < g.KW && c < g.C && f >= flo && f < fhi;
  uint32_t wd[4] = {0, 0, 0, 0};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int kb = 2 * s + (e >> 2);
    const int kap = kb * 16 + 4 * (lane >> 4) + (e & 3);
    float v = 0.f;
    if (ok && kb < g.NBLK) v = (float)to_i8_wrap(wslice(g, ws, f, kap));
    wd[e >> 1] |= (uint32_t)bf16_bits(v) << (16 * (e & 1));
  }
  v4i o;
  o.x = (int)wd[0]; o.y = (int)wd[1]; o.z = (int)wd[2]; o.w = (int)wd[3];
  wcy[t] = o;
}

// the weight operand of one (ob, pair t, K-step s, w-slice k) fragment, lane l: output channel
// o = ob*16 + (l & 15), byte e = w-slice k of weight (c = cb*16 + e, position p = 4s + (l >> 4)),
// rint(slice) as int8 as in wfrag_item; zero when p > 8 or the row f = c*9 + p is outside tile i
// wf5[((ob*ntc + t)*3 + s)*3 + k][64]
template <typename WS>
__device__ inline void wf5_item(const Geo& g, const F5W& v, const WS& ws, v4i* __restrict__ wf5, int t) {
  const int lane = t & 63;
  int r = t >> 6;
  const int k = r % 3;
  r /= 3;
  const int s = r % 3;
  r /= 3;
  const int tc = r % v.ntc;
  const int ob = r / v.ntc;
  int i = 0;
  while (v.tc0[i + 1] <= tc) ++i;
  const int flo = i * g.xbar, fhi = min(flo + g.xbar, g.K);
  const int p = 4 * s + (lane >> 4);
  const int n = k * g.Opad + ob * 16 + (lane & 15);
  uint32_t wd[4] = {0, 0, 0, 0};
  if (p < 9) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int c = v.tcb[tc] * 16 + e;
      const int f = c * 9 + p;
      int val = 0;
      if (c < g.C && f >= flo && f < fhi) val = clamp_i8(wslice(g, ws, f, n));
      wd[e >> 2] |= ((uint32_t)(uint8_t)(int8_t)val) << (8 * (e & 3));
    }
  }
  v4i o;
  o.x = (int)wd[0]; o.y = (int)wd[1]; o.z = (int)wd[2]; o.w = (int)wd[3];
  wf5[t] = o;
}

// weight operand of (tile i, output half h, position p, K-step s, input block cb), lane l: channel
// c = 16 cb + (l & 15), K values kappa = 32 s + 8 (l >> 4) + e (e < 8) = (k, o) = (kappa / 16, 16 h + kappa % 16),
// int8(slice_k) of weight (o, f = 9 c + p) as bf16 (wcy_item's values), zero for kappa >= 48 or f outside
// tile i: wg5[((((i * CBN + h) * 9 + p) * 2 + s) * CBN + cb) * 64 + l]
template <typename WS>
__device__ inline void wg5_item(const Geo& g, const WS& ws, v4i* __restrict__ wg5, int t) {
  const int CBN = g.C / 16;
  const int lane = t & 63;
  int r = t >> 6;
  const int cb = r % CBN;
  r /= CBN;
  const int s = r & 1;
  r >>= 1;
  const int p = r % 9;
  r /= 9;
  const int h = r % CBN, i = r / CBN;
  const int c = 16 * cb + (lane & 15);
  const int f = c * 9 + p;
  const int flo = i * g.xbar, fhi = min(flo + g.xbar, g.K);
  const bool ok = c < g.C && f >= flo && f < fhi;
  uint32_t wd[4] = {0, 0, 0, 0};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int kap = 32 * s + 8 * (lane >> 4) + e;
    const int k = kap >> 4, o = 16 * h + (kap & 15);
    float val = 0.f;
    if (ok && k < g.nbw) val = (float)to_i8_wrap(wslice(g, ws, f, k * g.Opad + o));
    wd[e >> 1] |= (uint32_t)bf16_bits(val) << (16 * (e & 1));
  }
  v4i q;
  q.x = (int)wd[0]; q.y = (int)wd[1]; q.z = (int)wd[2]; q.w = (int)wd[3];
  wg5[t] = q;
}

// the gx operand: lane l of (position p, K-step s): input channel c = l & 15, kappa = 32 s + 8 (l >> 4) + e
// (e < 8) = (tile i, w-slice k, output channel o) = (kappa / 48, (kappa % 48) / 16, kappa % 16), the value
// int8(slice_k) of weight (o, f = 9 c + p) as bf16 (the backward's ctx slice, lsq.py:160), zero unless row f is
// in tile i: wx6[(p * 3 + s) * 64 + l]
template <typename WS>
__device__ inline void wx6_item(const Geo& g, const WS& ws, v4i* __restrict__ wx6, int t) {
  const int lane = t & 63;
  const int r = t >> 6;
  const int s = r % kR6KSG, p = r / kR6KSG;
  const int c = lane & 15;
  const int f = c * 9 + p;
  uint32_t wd[4] = {0, 0, 0, 0};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int kap = 32 * s + 8 * (lane >> 4) + e;
    const int i = kap / kR6KO, rem = kap - i * kR6KO, k = rem >> 4, o = rem & 15;
    float val = 0.f;
    if (c < g.C && i < g.T && f >= i * g.xbar && f < min((i + 1) * g.xbar, g.K) && k < g.nbw)
      val = (float)to_i8_wrap(wslice(g, ws, f, k * g.Opad + o));
    wd[e >> 1] |= (uint32_t)bf16_bits(val) << (16 * (e & 1));
  }
  v4i q;
  q.x = (int)wd[0]; q.y = (int)wd[1]; q.z = (int)wd[2]; q.w = (int)wd[3];
  wx6[t] = q;
}

// =========================================================================================
// prep_params: ADC thresholds and STE intervals by exact binary search over integer ps
// =========================================================================================
// The ADC code and the STE mask are monotone step functions of the integer partial sum
// (each op in u = fp16(ps)*sw*sa, u/alpha, rint, clamp is monotone for sw*sa > 0 and
// alpha > 0), so they are captured exactly by integer thresholds found with the very
// same fp32 ops.  Anything else (alpha_q <= 0 / NaN -- e.g. all-equal alpha_cim gives
// NaN, lsq.py:570-571 -- or non-positive scales) sets flags[0]: kernels then evaluate
// the ADC literally per partial sum.
__device__ inline int first_true_ternary_hi(int lo, int hi, float sw, float sa, float a) {
  // smallest p in [lo, hi] with rint(u/a) >= 1 ; hi+1 if none
  int L = lo, R = hi + 1;
  while (L < R) {
    int mid = L + ((R - L) >> 1);
    float q = rintf(u_of(mid, sw, sa) / a);
    if (q >= 1.f) R = mid; else L = mid + 1;
  }
  return L;
}
__device__ inline int last_true_ternary_lo(int lo, int hi, float sw, float sa, float a) {
  // largest p in [lo, hi] with rint(u/a) <= -1 ; lo-1 if none
  int L = lo - 1, R = hi;
  while (L < R) {
    int mid = L + ((R - L + 1) >> 1);
    float q = rintf(u_of(mid, sw, sa) / a);
    if (q <= -1.f) L = mid; else R = mid - 1;
  }
  return L;
}

// Source of alpha_q: a materialised alpha_q, or alpha_cim through its quantiser in place
// (alpha_q = clamp(round_pass(a / scale), 1, 2^b - 1) * scale, lsq.py:566-571).
struct ASrc {
  const float* a;
  int raw;
  float scale, qp_al;
  __device__ float get(int e) const {
    if (!raw) return a[e];
    const float t = a[e] / scale;
    return clamp_nan(round_pass_value(t), 1.f, qp_al) * scale;
  }
};

__device__ inline bool scales_ok(float sw, float sa) {
  return (sw * sa > 0.f) && isfinite(sw * sa) && isfinite(sw) && isfinite(sa);
}

// one (i, j, k, o) entry (t < npar) or one (k, j) coefficient triple (t >= npar); returns
// whether the entry needs the literal ADC
__device__ inline bool params_item(const Geo& g, const ASrc& as, float sw, float sa,
                                   const int8_t* __restrict__ bmask, const Params& pp, int t,
                                   const float* __restrict__ beta = nullptr) {
  const int npar = g.T * g.nba * g.nbw * g.Opad;
  const int nkj = g.nbw * g.nba;
  if (t >= npar + nkj) {  // shift ADC: sum_{i,k,j} beta * mask of channel o, added to every output
    const int o = t - npar - nkj;
    float b = 0.f;
    if (beta != nullptr && o < g.O)
      for (int i = 0; i < g.T; ++i)
        for (int k = 0; k < g.nbw; ++k)
          for (int j = 0; j < g.nba; ++j)
            b += beta[((i * g.nbw + k) * g.nba + j) * g.O + o] * (float)bmask[k * g.nba + j];
    pp.bsum[o] = b;
    return false;
  }
  if (t >= npar) {  // per-(k,j) float coefficients
    const int kj = t - npar, k = kj / g.nba, j = kj - k * g.nba;
    const float mk = (float)bmask[k * g.nba + j];  // binary_mask[0,0,k,j,0,0]
    pp.ckj[kj] = mk;
    pp.ckj[nkj + kj] = mk * pow2f(-g.bsa * j);      // E weight: 2^-(bsa*j) * mask
    pp.ckj[2 * nkj + kj] = mk * pow2f(-g.bsw * k);  // D weight: 2^-(bsw*k) * mask
    return false;
  }
  int r = t;
  const int o = r % g.Opad; r /= g.Opad;
  const int k = r % g.nbw; r /= g.nbw;
  const int j = r % g.nba;
  const int i = r / g.nba;
  const float mk = (float)bmask[k * g.nba + j];
  float a = 1.f;
  if (has_alpha(g) && as.a != nullptr && o < g.O)
    a = as.get(((i * g.nbw + k) * g.nba + j) * g.O + o);  // alpha[0,i,k,j,0,o]
  pp.alpha[t] = a;
  pp.beta[t] = (beta != nullptr && o < g.O) ? beta[((i * g.nbw + k) * g.nba + j) * g.O + o] : 0.f;
  pp.coef[t] = a * mk;
  const int lo = -g.psmax - 1, hi = g.psmax + 1;
  bool literal = false;
  int thi = hi + 1, tlo = lo - 1, mlo = hi + 1, mhi = lo - 1;
  if (g.mode == ADC_SIGN || g.mode == ADC_TERNARY) {
    if (!(scales_ok(sw, sa) && a > 0.f && isfinite(a))) literal = true;
  }
  // the variants are evaluated per partial sum, except the shift ADC of the fast path
  const bool sf = shift_fast(g);
  const float be = pp.beta[t];
  if (g.variant != VAR_LIBRARY && !sf) literal = true;
  if (sf && !isfinite(be)) literal = true;
  if (!literal) {
    if (sf) {
      // v = (u - beta) / alpha (scale_shift.py:421): code +1 <=> rint(v) >= 1, -1 <=> rint(v) <= -1
      int L = lo, R = hi + 1;
      while (L < R) {
        const int mid = L + ((R - L) >> 1);
        if (rintf(psb_value(g, mid, sw, sa, a, be)) >= 1.f) R = mid; else L = mid + 1;
      }
      thi = L;
      L = lo - 1; R = hi;
      while (L < R) {
        const int mid = L + ((R - L + 1) >> 1);
        if (rintf(psb_value(g, mid, sw, sa, a, be)) <= -1.f) L = mid; else R = mid - 1;
      }
      tlo = L;
    } else if (g.mode == ADC_TERNARY) {
      thi = first_true_ternary_hi(lo, hi, sw, sa, a);
      tlo = last_true_ternary_lo(lo, hi, sw, sa, a);
    }
    // STE interval: psb(p) monotone non-decreasing in p
    {
      int L = lo, R = hi + 1;  // first p with psb > thr_lo  (i.e. not "<= thr_lo")
      while (L < R) {
        int mid = L + ((R - L) >> 1);
        float b = sf ? psb_value(g, mid, sw, sa, a, be) : psb_literal(mid, g.mode, sw, sa, a);
        if (b > g.thr_lo) R = mid; else L = mid + 1;
      }
      mlo = L;
      L = lo - 1; R = hi;  // last p with psb < thr_hi
      while (L < R) {
        int mid = L + ((R - L + 1) >> 1);
        float b = sf ? psb_value(g, mid, sw, sa, a, be) : psb_literal(mid, g.mode, sw, sa, a);
        if (b < g.thr_hi) L = mid; else R = mid - 1;
      }
      mhi = L;
    }
  }
  pp.thi[t] = thi;
  pp.tlo[t] = tlo;
  // STE interval as (lo, span): pass <=> (unsigned)(ps - lo) <= (unsigned)span
  if (mhi >= mlo) { pp.mlo[t] = mlo; pp.mhi[t] = mhi - mlo; }
  else { pp.mlo[t] = -(1 << 30); pp.mhi[t] = 0; }
  return literal;
}

}  // namespace cimq
