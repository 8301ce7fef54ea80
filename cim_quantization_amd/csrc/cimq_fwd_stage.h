// cimq_fwd_stage.h -- LDS staging of the activation patch and the operand gather shared by the forward
// kernels (cim_fwd_v3_kernel, cim_fwd5_kernel) and the recompute backward (cim_bwd_r6_kernel).
#pragma once
#include "cimq_operands.h"

namespace cimq {

// floor(n / d) for 0 <= n < 2^22 (inv = 1.f / d): float estimate + one correction step
__device__ inline int fdiv(int n, int d, float inv) {
  int q = (int)((float)n * inv);
  const int r = n - q * d;
  if (r < 0) q -= 1;
  else if (r >= d) q += 1;
  return q;
}

// Batched global -> LDS copy: every thread issues U independent loads before its first LDS
// store, so a block waits about one memory latency per U*blockDim elements instead of one
// per element.  src(idx) returns element idx; it lands in dst[idx].
template <int U, typename T, typename Src>
__device__ inline void batched_copy(int n, T* dst, Src src) {
  const int nt = blockDim.x;
  for (int base = threadIdx.x; base < n; base += U * nt) {
    T v[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (base + u * nt < n) v[u] = src(base + u * nt);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (base + u * nt < n) dst[base + u * nt] = v[u];
  }
}

// ---------------------------------------------------------------------------------------
// patch staging: rows [ih_first, ih_first + RHx) of image b -> LDS [C][RHx][WP] words of
// NBP bytes; data columns only (the 2*PW padding columns are zeroed once per block).  Rows
// outside the image are written as zeros.
// ---------------------------------------------------------------------------------------
__device__ inline void zero_lds(uint32_t* p, int nwords) {
  for (int t = threadIdx.x; t < nwords; t += blockDim.x) p[t] = 0u;
}

template <int NBP>
__device__ inline void stage_rows(const Geo& g, int WP, int RHx, const uint8_t* __restrict__ xc, int b,
                                  int ih_first, uint8_t* patch, int c0 = 0, int ncx = -1) {
  const int QW = g.W * NBP / 16;  // 16-byte vectors per row
  const int nrow = (ncx < 0 ? g.C : ncx) * RHx;
  const int n = nrow * QW;
  const uint4* src = reinterpret_cast<const uint4*>(xc) + ((size_t)b * g.C + c0) * g.H * QW;
  const int nt = blockDim.x;
  // item -> (row, q) by a shift when QW is a power of two, row -> (c, rr) by a 24-bit
  // multiply-shift (exact for row * RHx < 2^20); 32-bit offsets from the image's base: no
  // quarter-rate 32/64-bit multiplies per item
  const bool pq = (QW & (QW - 1)) == 0;
  const int lq = 31 - __builtin_clz(QW);
  const bool mag_ok = nrow * RHx < (1 << 20);
  const unsigned mag = ((1u << 20) + RHx - 1) / RHx;
  const float invQ = 1.f / (float)QW, invR = 1.f / (float)RHx;
  const int HQ = g.H * QW, rowb = WP * NBP, colb = g.PW * NBP;
  for (int base = threadIdx.x; base < n; base += 8 * nt) {
    uint4 v[8];
    int d[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + u * nt;
      d[u] = -1;
      if (idx < n) {
        const int row = pq ? (idx >> lq) : fdiv(idx, QW, invQ), q = pq ? (idx & (QW - 1)) : idx - row * QW;
        const int c = mag_ok ? (int)(__umul24((unsigned)row, mag) >> 20) : fdiv(row, RHx, invR);
        const int rr = row - c * RHx;
        const int ih = ih_first + rr;
        d[u] = row * rowb + colb + q * 16;
        v[u] = make_uint4(0, 0, 0, 0);
        if ((unsigned)ih < (unsigned)g.H) v[u] = src[c * HQ + ih * QW + q];
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (d[u] >= 0) {
        uint32_t* p = reinterpret_cast<uint32_t*>(patch + d[u]);
        p[0] = v[u].x; p[1] = v[u].y; p[2] = v[u].z; p[3] = v[u].w;
      }
    }
  }
}

// stage_rows for the module forward with the LSQ activation quantiser fused (NBP 4): the rows are read
// as fp32 x and turned into slice words on the way into LDS -- act_words_lut, the same table and the
// same element chain as the prologue's act_range, so the words are bit-identical -- and the block
// that owns input rows [own_lo, own_hi) also writes their backward (ctx) words to xcb.  The forward
// slice words are never stored.
// lut: [Qp + 1][fwd, bwd] from act_lut_build plus, at entry Qp + 1, the words of a NaN element
// (act_words of any NaN: every step of its chain is independent of the NaN's sign and payload)
__device__ inline uint2 act_words_tab(float v, float sa, float qp, int nan_e, const uint32_t* lut) {
  const float c = clamp_nan(v / sa, 0.f, qp);
  const float r = rintf(c);
  const int e = (r == r) ? (int)r : nan_e;
  return *reinterpret_cast<const uint2*>(lut + 2 * e);
}
template <int NBA_C>
__device__ inline void act_lut_build_q(const Geo& g, float sa, bool sgn, uint32_t* lut) {
  if (threadIdx.x == 0) {
    uint32_t f[1], b[1];
    act_words<4, NBA_C>(g, __int_as_float(0x7fc00000), sa, sgn, f, b);
    const int e = (int)g.lsq_qp + 1;
    lut[2 * e] = f[0];
    lut[2 * e + 1] = b[0];
  }
  act_lut_build<4, NBA_C>(g, sa, sgn, lut);  // entries 0 .. Qp, then the block barrier
}
// WCB false (forward only): no backward words at all, xcb is not read
template <bool WCB = true>
__device__ inline void stage_rows_q(const Geo& g, int WP, int RHx, const float* __restrict__ x, float sa,
                                    const uint32_t* lut, int b, int ih_first, uint8_t* patch,
                                    uint8_t* __restrict__ xcb, int own_lo, int own_hi) {
  const int nan_e = (int)g.lsq_qp + 1;
  const int QW = g.W >> 2;  // 4-element items per row (W % 4 == 0)
  const int nrow = g.C * RHx;
  const int n = nrow * QW;
  const bool pq = (QW & (QW - 1)) == 0;
  const int lq = 31 - __builtin_clz(QW);
  const float invQ = 1.f / (float)QW, invR = 1.f / (float)RHx;
  const size_t img = (size_t)b * g.C * g.H;
  for (int base = threadIdx.x; base < n; base += 4 * (int)blockDim.x) {
    float4 v[4];
    int d[4], ihs[4], cs[4], qs[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = base + u * (int)blockDim.x;
      d[u] = -1;
      if (idx < n) {
        const int row = pq ? (idx >> lq) : fdiv(idx, QW, invQ), q = pq ? (idx & (QW - 1)) : idx - row * QW;
        const int c = fdiv(row, RHx, invR);
        const int ih = ih_first + (row - c * RHx);
        d[u] = row * WP * 4 + g.PW * 4 + q * 16;
        ihs[u] = ih;
        cs[u] = c;
        qs[u] = q;
        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((unsigned)ih < (unsigned)g.H)
          v[u] = reinterpret_cast<const float4*>(x)[((img + (size_t)c * g.H + ih) * g.W >> 2) + q];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (d[u] < 0) continue;
      uint32_t* p = reinterpret_cast<uint32_t*>(patch + d[u]);
      if ((unsigned)ihs[u] >= (unsigned)g.H) {
        p[0] = p[1] = p[2] = p[3] = 0u;
        continue;
      }
      const uint2 w0 = act_words_tab(v[u].x, sa, g.lsq_qp, nan_e, lut);
      const uint2 w1 = act_words_tab(v[u].y, sa, g.lsq_qp, nan_e, lut);
      const uint2 w2 = act_words_tab(v[u].z, sa, g.lsq_qp, nan_e, lut);
      const uint2 w3 = act_words_tab(v[u].w, sa, g.lsq_qp, nan_e, lut);
      p[0] = w0.x; p[1] = w1.x; p[2] = w2.x; p[3] = w3.x;
      if constexpr (!WCB) continue;
      if (ihs[u] >= own_lo && ihs[u] < own_hi)
        reinterpret_cast<uint4*>(xcb)[((img + (size_t)cs[u] * g.H + ihs[u]) * g.W >> 2) + qs[u]] =
            make_uint4(w0.y, w1.y, w2.y, w3.y);
    }
  }
}

// stage_rows_q<false> for eight slices a side (NBP 8: the w8a8 first conv, 8-byte patch words): no table -- a signed
// activation's codes are not table indices -- but act_words itself on every element, the chain prep_module_fwd_kernel
// runs (its table holds act_words_xq of r * sa, which is what act_words makes of an element whose code is r), so the
// patch holds that prologue's forward words bit for bit.  Eight 1-bit slices and W % 4 == 0 (fwd8_stage_ok).
__device__ inline void stage_rows_q8(const Geo& g, int WP, int RHx, const float* __restrict__ x, float sa, bool sgn,
                                     int b, int ih_first, uint8_t* patch) {
  const int QW = g.W >> 2;  // 4-element items per row
  const int n = g.C * RHx * QW;
  const float invQ = 1.f / (float)QW, invR = 1.f / (float)RHx;
  const size_t img = (size_t)b * g.C * g.H;
  for (int idx = threadIdx.x; idx < n; idx += (int)blockDim.x) {
    const int row = fdiv(idx, QW, invQ), q = idx - row * QW;
    const int c = fdiv(row, RHx, invR);
    const int ih = ih_first + (row - c * RHx);
    // (8-byte stores: the padding columns leave a row's data 8-byte aligned only)
    uint2* p = reinterpret_cast<uint2*>(patch + ((size_t)row * WP + g.PW) * 8 + q * 32);
    if ((unsigned)ih >= (unsigned)g.H) {
      p[0] = p[1] = p[2] = p[3] = make_uint2(0u, 0u);
      continue;
    }
    const float4 v = reinterpret_cast<const float4*>(x)[((img + (size_t)c * g.H + ih) * g.W >> 2) + q];
    uint32_t f0[2], f1[2], f2[2], f3[2], bw[2];
    act_words<8, 8>(g, v.x, sa, sgn, f0, bw);
    act_words<8, 8>(g, v.y, sa, sgn, f1, bw);
    act_words<8, 8>(g, v.z, sa, sgn, f2, bw);
    act_words<8, 8>(g, v.w, sa, sgn, f3, bw);
    p[0] = make_uint2(f0[0], f0[1]);
    p[1] = make_uint2(f1[0], f1[1]);
    p[2] = make_uint2(f2[0], f2[1]);
    p[3] = make_uint2(f3[0], f3[1]);
  }
}

// stage_rows_q for an input that arrives as activation codes (cimq_module_forward_codes; forward only, so no
// backward words): one byte per element, [B, C, H, W], four columns per 32-bit load, each byte straight into the
// word table -- no division, clamp or rint.  A byte above Qp + 1 reads the NaN entry: none indexes past the table.
__device__ inline void stage_rows_qc(const Geo& g, int WP, int RHx, const uint8_t* __restrict__ xq,
                                     const uint32_t* lut, int b, int ih_first, uint8_t* patch) {
  const int nan_e = (int)g.lsq_qp + 1;
  const int QW = g.W >> 2;  // 4-element items per row (W % 4 == 0)
  const int nrow = g.C * RHx;
  const int n = nrow * QW;
  const bool pq = (QW & (QW - 1)) == 0;
  const int lq = 31 - __builtin_clz(QW);
  const float invQ = 1.f / (float)QW, invR = 1.f / (float)RHx;
  const size_t img = (size_t)b * g.C * g.H;
  for (int base = threadIdx.x; base < n; base += 4 * (int)blockDim.x) {
    uint32_t v[4];
    int d[4];
    bool in[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = base + u * (int)blockDim.x;
      d[u] = -1;
      v[u] = 0u;
      in[u] = false;
      if (idx < n) {
        const int row = pq ? (idx >> lq) : fdiv(idx, QW, invQ), q = pq ? (idx & (QW - 1)) : idx - row * QW;
        const int c = fdiv(row, RHx, invR);
        const int ih = ih_first + (row - c * RHx);
        d[u] = row * WP * 4 + g.PW * 4 + q * 16;
        in[u] = (unsigned)ih < (unsigned)g.H;
        if (in[u]) v[u] = reinterpret_cast<const uint32_t*>(xq)[((img + (size_t)c * g.H + ih) * g.W >> 2) + q];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (d[u] < 0) continue;
      uint32_t* p = reinterpret_cast<uint32_t*>(patch + d[u]);
#pragma unroll
      for (int e = 0; e < 4; ++e) p[e] = in[u] ? lut[2 * min((int)((v[u] >> (8 * e)) & 255u), nan_e)] : 0u;
    }
  }
}

// ptab[t] (t < KS*64) for tile i: patch word offset of contraction row f = i*xbar + t relative
// to a pixel's window origin; 0 for t outside the tile (the weight operand is zero there).
__device__ inline void build_ptab(const Geo& g, int i, int KSx, int RHx, int WP, int* ptab, int c0 = 0) {
  for (int t = threadIdx.x; t < KSx * 64; t += blockDim.x) {
    const int f = i * g.xbar + t;
    int off = 0;
    if (t < g.xbar && f < g.K) {
      const int c = fdiv(f, g.KHW, 1.f / (float)g.KHW), rem = f - c * g.KHW;
      const int kh = fdiv(rem, g.KW, 1.f / (float)g.KW), kw = rem - kh * g.KW;
      off = ((c - c0) * RHx + kh) * WP + kw;
    }
    ptab[t] = off;
  }
}

// 4x4 byte transpose: P_j byte e = w_e byte j
__device__ inline void tr4(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t (&P)[4]) {
  const uint32_t t01l = __builtin_amdgcn_perm(w1, w0, 0x05010400u);
  const uint32_t t01h = __builtin_amdgcn_perm(w1, w0, 0x07030602u);
  const uint32_t t23l = __builtin_amdgcn_perm(w3, w2, 0x05010400u);
  const uint32_t t23h = __builtin_amdgcn_perm(w3, w2, 0x07030602u);
  P[0] = __builtin_amdgcn_perm(t23l, t01l, 0x05040100u);
  P[1] = __builtin_amdgcn_perm(t23l, t01l, 0x07060302u);
  P[2] = __builtin_amdgcn_perm(t23h, t01h, 0x05040100u);
  P[3] = __builtin_amdgcn_perm(t23h, t01h, 0x07060302u);
}

// The int8 MFMA operand of one pixel (this lane's column / row l&15) for tile i:
// xs[j][ks] byte e = slice j of the element at contraction index t = ks*64 + 16*(l>>4) + e.
template <int NBP, int KS>
__device__ inline void gather_xs(const uint8_t* patch, int rb, const int* ptab, int g4, v4i (&xs)[NBP][KS],
                                 int ksn = KS) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    if (ks >= ksn) break;
    const int4* pt = reinterpret_cast<const int4*>(ptab + ks * 64 + 16 * g4);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int4 o4 = pt[q];
      const int oo[4] = {o4.x, o4.y, o4.z, o4.w};
      uint32_t w[4], wh[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (NBP == 4) {
          w[e] = reinterpret_cast<const uint32_t*>(patch)[rb + oo[e]];
        } else {
          const uint2 t = reinterpret_cast<const uint2*>(patch)[rb + oo[e]];
          w[e] = t.x;
          wh[e] = t.y;
        }
      }
      uint32_t P[4];
      tr4(w[0], w[1], w[2], w[3], P);
#pragma unroll
      for (int j = 0; j < 4; ++j) xs[j][ks][q] = (int)P[j];
      if (NBP == 8) {
        tr4(wh[0], wh[1], wh[2], wh[3], P);
#pragma unroll
        for (int j = 0; j < 4; ++j) xs[4 + j][ks][q] = (int)P[j];
      }
    }
  }
}

// act_words_tab's table entry with the clamp moved after the rounding (rint(clamp(q, 0, Qp)) = clamp(rint(q),
// 0, Qp) for integer bounds): v_cvt_i32_f32 saturates +-inf and the NaN test picks the table's NaN entry
__device__ inline uint2 act_words_q5(float v, float sa, int qp, int nan_e, const uint32_t* lut, int& code) {
  const float q = v / sa;
  int e;
  asm("v_cvt_i32_f32 %0, %1" : "=v"(e) : "v"(rintf(q)));
  e = min(max(e, 0), qp);
  e = (q == q) ? e : nan_e;
  code = e;
  return *reinterpret_cast<const uint2*>(lut + 2 * e);
}

// n / d for 0 <= n < 2^20, d < 2^10 (inv = 1 / d in fp32): exact, no correction step needed
__device__ inline int sdiv(int n, float inv) { return (int)(((float)n + 0.5f) * inv); }

// LDS byte offset of the patch element (row, channel-block slot, col) of one image slot, slice 0
// (slice j at + 16 j)
__device__ inline int f5_off(int NCB, int WP, int row, int cb, int col) { return ((row * NCB + cb) * WP + col) * 48; }

}  // namespace cimq
