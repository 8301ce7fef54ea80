// cimq_ideal.hip -- the ideal-ADC conv, Conv2dLSQCiM(adcbits = 0) (lsq.py:584-585): LSQ codes on both sides, no
// partial-sum quantisation, so nothing cuts the contraction into crossbar tiles or slice pairs.
//   forward : out = conv(code_a, code_w) * sa * sw, one int32 accumulation over all of C * KH * KW on
//             v_mfma_i32_16x16x64_i8; x is quantised in the row staging (bytes in LDS, channels contiguous)
//   backward: the code operand (|code| <= 255) is exact in ONE bf16 value and only grad_out needs the hi / mid / lo
//             split, so each product is three v_mfma_f32_16x16x32_bf16 with fp32 accuracy and no state words:
//             grad_x contracts (kh, kw, o) against the transposed weight codes, grad_w contracts the pixels against
//             the activation codes requantised from x; the LSQ step-size sums ride on both epilogues.
// No atomics: every sum has a fixed order.  Included by cimq_part_ideal.hip; plans in cimq_host.h (ideal_plan).
#pragma once
#include "cimq_ideal_dev.h"

namespace cimq {

// ---------------------------------------------------------------------------------------
// weight side, once per forward: the codes as int8 A-fragments of the forward
//   wf[((ch * fks + ks) * nob + ob) * 64 + lane]: row o = ob*16 + (lane & 15), k = ks*64 + 16*(lane >> 4) + e
//   = (tap * (ncx/16) + cg) * 16 + e of channel chunk ch: channel ch*ncx + cg*16 + e of tap (kh, kw)
// and, unless inference, as bf16 A-fragments of grad_x (the transposed operand)
//   wx[(((cb * xnoch + och) * xks + ks) * 64 + lane]: row c = cb*16 + (lane & 15), k = ks*32 + 8*(lane >> 4) + e
//   = (tap * (noc/8) + o8) * 8 + e of output chunk och: output channel och*noc + o8*8 + e
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ideal_prep_w_kernel(IdealG g, const float* __restrict__ w,
                                                           const float* __restrict__ alpha_w, v4i* __restrict__ wf,
                                                           v4i* __restrict__ wx) {
  const float sw = grad_scale_value(alpha_w[0], g.gw);
  const int nwf = g.nch * g.fks * g.nob * 64;
  const int nwx = g.inference ? 0 : g.ncb * g.xnoch * g.xks * 64;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < nwf + nwx; t += gridDim.x * blockDim.x) {
    uint32_t wd[4] = {0u, 0u, 0u, 0u};
    if (t < nwf) {
      const int lane = t & 63, r = t >> 6;
      const int ob = r % g.nob, r2 = r / g.nob;
      const int ks = r2 % g.fks, ch = r2 / g.fks;
      const int o = ob * 16 + (lane & 15);
      const int kc = ks * 4 + (lane >> 4), g16 = g.ncx >> 4;
      const int tap = kc / g16, cg = kc - tap * g16;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int c = ch * g.ncx + cg * 16 + e;
        int v = 0;
        if (o < g.O && c < g.C && tap < g.ntap)
          v = (int)ideal_code(w[((size_t)o * g.C + c) * g.ntap + tap], sw, g.qn_w, g.qp_w);
        wd[e >> 2] |= ((uint32_t)(uint8_t)(int8_t)v) << (8 * (e & 3));
      }
      wf[t] = v4i{(int)wd[0], (int)wd[1], (int)wd[2], (int)wd[3]};
    } else {
      const int u = t - nwf;
      const int lane = u & 63, r = u >> 6;
      const int ks = r % g.xks, r2 = r / g.xks;
      const int och = r2 % g.xnoch, cb = r2 / g.xnoch;
      const int c = cb * 16 + (lane & 15);
      const int kc = ks * 4 + (lane >> 4), g8 = g.noc >> 3;
      const int tap = kc / g8, o8 = kc - tap * g8;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int o = och * g.noc + o8 * 8 + e;
        float v = 0.f;
        if (o < g.O && c < g.C && tap < g.ntap)
          v = ideal_code(w[((size_t)o * g.C + c) * g.ntap + tap], sw, g.qn_w, g.qp_w);
        wd[e >> 1] |= (__float_as_uint(v) >> 16) << (16 * (e & 1));  // |v| <= 128: exact in bf16
      }
      wx[u] = v4i{(int)wd[0], (int)wd[1], (int)wd[2], (int)wd[3]};
    }
  }
}

// ---------------------------------------------------------------------------------------
// forward.  Workgroup = one 64-pixel m-tile of one image (blockIdx.x) x NOB 16-channel output blocks (blockIdx.y);
// wave w owns pixels 16 w .. 16 w + 15 of the tile.  Per channel chunk: the input rows the tile reads are quantised
// into the LDS patch [row][col + PW][channel] (bytes; fpitch per pixel), then every 64-deep k-step is one
// ds_read_b128 per lane (16 channels of one tap, offset from the tap table) and NOB MFMAs against fragments from ctx.
// LDS: tap table [fks * 4] ints | patch.
// ---------------------------------------------------------------------------------------
template <int NOB, bool SPLIT>
__global__ __launch_bounds__(256) void cim_ideal_fwd_kernel(IdealG g, const float* __restrict__ x,
                                                            const v4i* __restrict__ wf,
                                                            const float* __restrict__ alpha_a,
                                                            const float* __restrict__ alpha_w,
                                                            float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  int* tab = reinterpret_cast<int*>(lds);
  uint8_t* patch = lds + ((g.fks * 16 + 15) & ~15);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, g4 = lane >> 4;
  const int b = blockIdx.x / g.mt, p0 = (blockIdx.x - b * g.mt) * 64;
  const int ob0 = blockIdx.y * NOB;
  const float sa = grad_scale_value(alpha_a[0], g.ga);
  const int oh0 = p0 / g.Wo, oh1 = min(p0 + 63, g.P - 1) / g.Wo;
  const int nr = (oh1 - oh0) * g.SH + g.KH;  // <= g.frows
  const int ihb = oh0 * g.SH - g.PH;
  const int g16 = g.ncx >> 4;
  for (int kc = tid; kc < g.fks * 4; kc += 256) {
    const int tap = kc / g16, cg = kc - tap * g16;
    const int kh = tap / g.KW, kw = tap - kh * g.KW;
    tab[kc] = tap < g.ntap ? (kh * g.fwp + kw) * g.fpitch + cg * 16 : -1;
  }
  const int pl = p0 + wave * 16 + r16;
  const bool valid = pl < g.P;
  const int p = valid ? pl : g.P - 1;  // (a masked lane reads the last pixel's patch: in bounds)
  const int oh = p / g.Wo, ow = p - oh * g.Wo;
  const int base = ((oh - oh0) * g.SH * g.fwp + ow * g.SW) * g.fpitch;
  v4i acc[NOB], acch[NOB];
#pragma unroll
  for (int nb = 0; nb < NOB; ++nb) {
    acc[nb] = v4i{0, 0, 0, 0};
    acch[nb] = v4i{0, 0, 0, 0};
  }
  const int items = (g.ncx >> 2) * nr * g.fwp;
  for (int ch = 0; ch < g.nch; ++ch) {
    __syncthreads();  // the previous chunk's reads
    for (int it = tid; it < items; it += 256) {
      const int colp = it % g.fwp, t2 = it / g.fwp;
      const int row = t2 % nr, c4 = t2 / nr;
      const int ih = ihb + row, iw = colp - g.PW;
      uint32_t wd = 0u;
      if (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = ch * g.ncx + c4 * 4 + j;
          if (c < g.C) {
            const float v = x[(((size_t)b * g.C + c) * g.H + ih) * g.W + iw];
            wd |= ((uint32_t)(int)ideal_code(v, sa, 0.f, g.qp_a)) << (8 * j);
          }
        }
      }
      *reinterpret_cast<uint32_t*>(patch + (size_t)(row * g.fwp + colp) * g.fpitch + c4 * 4) = wd;
    }
    __syncthreads();
    const v4i* wfc = wf + ((size_t)ch * g.fks * g.nob + ob0) * 64 + lane;
    for (int ks = 0; ks < g.fks; ++ks) {
      const int off = tab[ks * 4 + g4];
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (off >= 0) v = *reinterpret_cast<const uint4*>(patch + base + off);
      v4i bl, bh;
      if (SPLIT) {
        bl = v4i{(int)(v.x & 0x0F0F0F0Fu), (int)(v.y & 0x0F0F0F0Fu), (int)(v.z & 0x0F0F0F0Fu), (int)(v.w & 0x0F0F0F0Fu)};
        bh = v4i{(int)((v.x >> 4) & 0x0F0F0F0Fu), (int)((v.y >> 4) & 0x0F0F0F0Fu), (int)((v.z >> 4) & 0x0F0F0F0Fu),
                 (int)((v.w >> 4) & 0x0F0F0F0Fu)};
      } else {
        bl = v4i{(int)v.x, (int)v.y, (int)v.z, (int)v.w};
        bh = bl;
      }
#pragma unroll
      for (int nb = 0; nb < NOB; ++nb) {
        if (ob0 + nb < g.nob) {
          const v4i a = wfc[((size_t)ks * g.nob + nb) * 64];
          acc[nb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bl, acc[nb], 0, 0, 0);
          if (SPLIT) acch[nb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bh, acch[nb], 0, 0, 0);
        }
      }
    }
  }
  if (!valid) return;
  const float sw = grad_scale_value(alpha_w[0], g.gw);
#pragma unroll
  for (int nb = 0; nb < NOB; ++nb) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = (ob0 + nb) * 16 + 4 * g4 + r;
      if (o < g.O) {
        const int iv = SPLIT ? acc[nb][r] + 16 * acch[nb][r] : acc[nb][r];
        out[((size_t)b * g.O + o) * g.P + p] = ((float)iv * sa) * sw;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// grad_x.  Workgroup = (image, band of xrb input rows x xwb columns; blockIdx.x) x kIdealCBX input-channel blocks
// (blockIdx.y).  Per output-channel chunk the grad_out rows the band reads are staged as three bf16 planes
// [row][col][o] (xopitch per pixel); the contraction over (kh, kw, o) runs 32 deep, a lane's 8 k being 8 output
// channels of one tap at the output pixel its input pixel meets under that tap (none: zero; stride 2 and the borders
// are this predicate).  D[c][pixel]: the epilogue multiplies by sw, re-derives x / sa, applies the clamp mask and
// leaves one act-LSQ partial per workgroup.  LDS: tap table [xks * 4] ints | hi | mid | lo.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cim_ideal_gx_kernel(IdealG g, const float* __restrict__ x,
                                                           const float* __restrict__ gout,
                                                           const v4i* __restrict__ wx,
                                                           const float* __restrict__ alpha_a,
                                                           const float* __restrict__ alpha_w, float* __restrict__ gx,
                                                           float* __restrict__ part_a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  __shared__ float red[4];
  int* tab = reinterpret_cast<int*>(lds);
  const size_t plane = (size_t)g.xrows * g.Wo * g.xopitch * 2;
  uint8_t* pl0 = lds + ((g.xks * 16 + 15) & ~15);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, g4 = lane >> 4;
  int bx = blockIdx.x;
  const int colb = bx % g.xncol; bx /= g.xncol;
  const int rb = bx % g.xnrb, b = bx / g.xnrb;
  const int ih0 = rb * g.xrb, iw0 = colb * g.xwb;
  const int cb0 = blockIdx.y * kIdealCBX;
  // grad_out rows oh with oh * SH in [ih0 + PH - KH + 1, ih0 + xrb - 1 + PH]: at most g.xrows of them
  const int nlo = ih0 + g.PH - g.KH + 1;
  const int oh_lo = nlo <= 0 ? 0 : (nlo + g.SH - 1) / g.SH;
  const int oh_hi = min(g.Ho - 1, (ih0 + g.xrb - 1 + g.PH) / g.SH);
  const int ng = max(0, oh_hi - oh_lo + 1);
  const int g8 = g.noc >> 3;
  for (int kc = tid; kc < g.xks * 4; kc += 256) {
    const int tap = kc / g8, o8 = kc - tap * g8;
    const int kh = tap / g.KW, kw = tap - kh * g.KW;
    tab[kc] = tap < g.ntap ? (kh | (kw << 8) | ((o8 * 8) << 16)) : -1;
  }
  const int npix = g.xrb * g.xwb;  // <= 16 * 4 * kIdealPGX
  int ih[kIdealPGX], iw[kIdealPGX];
  bool pv[kIdealPGX];
#pragma unroll
  for (int q = 0; q < kIdealPGX; ++q) {
    const int idx = (wave + 4 * q) * 16 + r16;
    const int r = idx / g.xwb;
    ih[q] = ih0 + r;
    iw[q] = iw0 + (idx - r * g.xwb);
    pv[q] = idx < npix && ih[q] < g.H && iw[q] < g.W;
  }
  v4f acc[kIdealPGX][kIdealCBX];
#pragma unroll
  for (int q = 0; q < kIdealPGX; ++q)
#pragma unroll
    for (int cbi = 0; cbi < kIdealCBX; ++cbi) acc[q][cbi] = v4f{0.f, 0.f, 0.f, 0.f};
  const int sshift_h = g.SH - 1, sshift_w = g.SW - 1;  // strides 1 and 2
  const int items = (g.noc >> 1) * ng * g.Wo;
  for (int och = 0; och < g.xnoch; ++och) {
    __syncthreads();
    for (int it = tid; it < items; it += 256) {
      const int pix = it % (ng * g.Wo), o2 = it / (ng * g.Wo);
      const int o = och * g.noc + o2 * 2;
      const size_t gi = ((size_t)b * g.O + o) * g.P + (size_t)oh_lo * g.Wo + pix;
      const float a = o < g.O ? gout[gi] : 0.f;
      const float c = o + 1 < g.O ? gout[gi + g.P] : 0.f;
      uint32_t hi, mid, lo;
      split3_pk(a, c, hi, mid, lo);
      const size_t at = ((size_t)pix * g.xopitch + o2 * 2) * 2;
      *reinterpret_cast<uint32_t*>(pl0 + at) = hi;
      *reinterpret_cast<uint32_t*>(pl0 + plane + at) = mid;
      *reinterpret_cast<uint32_t*>(pl0 + 2 * plane + at) = lo;
    }
    __syncthreads();
    for (int ks = 0; ks < g.xks; ++ks) {
      const int e = tab[ks * 4 + g4];
      v4i a[kIdealCBX];
#pragma unroll
      for (int cbi = 0; cbi < kIdealCBX; ++cbi) {
        a[cbi] = v4i{0, 0, 0, 0};
        if (cb0 + cbi < g.ncb) a[cbi] = wx[(((size_t)(cb0 + cbi) * g.xnoch + och) * g.xks + ks) * 64 + lane];
      }
#pragma unroll
      for (int q = 0; q < kIdealPGX; ++q) {
        if ((wave + 4 * q) * 16 >= npix) continue;  // (wave-uniform)
        v4i bh = v4i{0, 0, 0, 0}, bm = bh, bl = bh;
        if (e >= 0 && pv[q]) {
          const int kh = e & 0xFF, kw = (e >> 8) & 0xFF, o8 = e >> 16;
          const int nh = ih[q] + g.PH - kh, nw = iw[q] + g.PW - kw;
          const int oh = nh >> sshift_h, ow = nw >> sshift_w;
          if (nh >= 0 && nw >= 0 && (nh & sshift_h) == 0 && (nw & sshift_w) == 0 && oh >= oh_lo && oh <= oh_hi &&
              ow < g.Wo) {
            const size_t at = ((size_t)((oh - oh_lo) * g.Wo + ow) * g.xopitch + o8) * 2;
            bh = *reinterpret_cast<const v4i*>(pl0 + at);
            bm = *reinterpret_cast<const v4i*>(pl0 + plane + at);
            bl = *reinterpret_cast<const v4i*>(pl0 + 2 * plane + at);
          }
        }
#pragma unroll
        for (int cbi = 0; cbi < kIdealCBX; ++cbi) {
          if (cb0 + cbi < g.ncb) {
            acc[q][cbi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_v8bf(a[cbi]), as_v8bf(bh), acc[q][cbi], 0, 0, 0);
            acc[q][cbi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_v8bf(a[cbi]), as_v8bf(bm), acc[q][cbi], 0, 0, 0);
            acc[q][cbi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_v8bf(a[cbi]), as_v8bf(bl), acc[q][cbi], 0, 0, 0);
          }
        }
      }
    }
  }
  const float sa = grad_scale_value(alpha_a[0], g.ga), sw = grad_scale_value(alpha_w[0], g.gw);
  float ps = 0.f;
#pragma unroll
  for (int q = 0; q < kIdealPGX; ++q) {
    if (!pv[q]) continue;
#pragma unroll
    for (int cbi = 0; cbi < kIdealCBX; ++cbi) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = (cb0 + cbi) * 16 + 4 * g4 + r;
        if (c < g.C) {
          const size_t xi = (((size_t)b * g.C + c) * g.H + ih[q]) * g.W + iw[q];
          const float t = x[xi] / sa;
          const bool inside = t >= 0.f && t <= g.qp_a;
          const float dq = acc[q][cbi][r] * sw;  // d loss / d x_q
          gx[xi] = inside ? dq : 0.f;
          const float code = rintf(fminf(fmaxf(t, 0.f), g.qp_a));
          ps += dq * (code - (inside ? t : 0.f));
        }
      }
    }
  }
  const float tot = ideal_block_sum(ps, red);
  if (tid == 0) part_a[blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

// ---------------------------------------------------------------------------------------
// grad_w.  Workgroup = slab (blockIdx.x: wupc units, a unit = wrb output rows of one image) x (input block, tap group;
// blockIdx.y) x kIdealOBG output blocks (blockIdx.z).  Per unit: grad_out rows as three bf16 planes [o][pixel]
// (pixels contiguous, rows padded to 8: a lane's 8 k are 8 consecutive output pixels of one row) and the x rows they
// meet as codes in bf16 (exact) [c][row][col + PW]; wave w contracts the 32-pixel steps w, w + 4, ...; for each tap of
// the group the B operand is the code row shifted by (kh, kw).  The four waves' sums meet in LDS in wave order and
// the workgroup writes its part of slab [o][tap][c].  LDS: x codes | hi | mid | lo, reused for the wave sums.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cim_ideal_gw_kernel(IdealG g, const float* __restrict__ x,
                                                           const float* __restrict__ gout,
                                                           const float* __restrict__ alpha_a,
                                                           float* __restrict__ slab) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  uint16_t* xs = reinterpret_cast<uint16_t*>(lds);
  const size_t xbytes = ((size_t)16 * g.wxplane * 2 + 15) & ~(size_t)15;
  const size_t plane = (size_t)16 * kIdealOBG * g.wgpitch * 2;
  uint8_t* gp = lds + xbytes;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, g4 = lane >> 4;
  const int cb = blockIdx.y / g.wntg, tg = blockIdx.y - cb * g.wntg;
  const int obp = blockIdx.z;
  const int t0 = tg * kIdealTG, tcount = min(kIdealTG, g.ntap - t0);
  const float sa = grad_scale_value(alpha_a[0], g.ga);
  int toff[kIdealTG];
#pragma unroll
  for (int i = 0; i < kIdealTG; ++i) {
    const int t = min(t0 + i, g.ntap - 1);
    const int kh = t / g.KW, kw = t - kh * g.KW;
    toff[i] = kh * g.wxw + kw;
  }
  v4f acc[kIdealTG][kIdealOBG];
#pragma unroll
  for (int i = 0; i < kIdealTG; ++i)
#pragma unroll
    for (int ol = 0; ol < kIdealOBG; ++ol) acc[i][ol] = v4f{0.f, 0.f, 0.f, 0.f};
  const int nseg = g.wrb * g.wspr, nks = (nseg + 3) >> 2;
  const int rowpix = g.wspr * 8;
  const int units = g.B * g.wnb;
  const int u1 = min(units, (int)(blockIdx.x + 1) * g.wupc);
  for (int u = blockIdx.x * g.wupc; u < u1; ++u) {
    const int b = u / g.wnb, oh0 = (u - b * g.wnb) * g.wrb;
    const int nrb = min(g.wrb, g.Ho - oh0);
    __syncthreads();
    for (int it = tid; it < 16 * g.wxrows * g.wxw; it += 256) {
      const int col = it % g.wxw, t2 = it / g.wxw;
      const int row = t2 % g.wxrows, cl = t2 / g.wxrows;
      const int c = cb * 16 + cl, ih = oh0 * g.SH - g.PH + row, iw = col - g.PW;
      float v = 0.f;
      if (c < g.C && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W)
        v = ideal_code(x[(((size_t)b * g.C + c) * g.H + ih) * g.W + iw], sa, 0.f, g.qp_a);
      xs[cl * g.wxplane + row * g.wxw + col] = (uint16_t)(__float_as_uint(v) >> 16);  // an integer <= 255: exact
    }
    for (int it = tid; it < 16 * kIdealOBG * g.wrb * rowpix; it += 256) {
      const int ow = it % rowpix, t2 = it / rowpix;
      const int r = t2 % g.wrb, ol = t2 / g.wrb;
      const int o = obp * 16 * kIdealOBG + ol;
      float v = 0.f;
      if (o < g.O && r < nrb && ow < g.Wo) v = gout[(((size_t)b * g.O + o) * g.Ho + oh0 + r) * g.Wo + ow];
      uint16_t hi, mid, lo;
      split3(v, hi, mid, lo);
      const size_t at = ((size_t)ol * g.wgpitch + r * rowpix + ow) * 2;
      *reinterpret_cast<uint16_t*>(gp + at) = hi;
      *reinterpret_cast<uint16_t*>(gp + plane + at) = mid;
      *reinterpret_cast<uint16_t*>(gp + 2 * plane + at) = lo;
    }
    __syncthreads();
    for (int ks = wave; ks < nks; ks += 4) {
      const int seg = ks * 4 + g4;
      const bool sv = seg < nseg;
      const int sc = sv ? seg : nseg - 1;
      const int r = sc / g.wspr, s8 = sc - r * g.wspr;
      v4i a[kIdealOBG][3];
#pragma unroll
      for (int ol = 0; ol < kIdealOBG; ++ol) {
        const size_t at = ((size_t)(ol * 16 + r16) * g.wgpitch + sc * 8) * 2;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          a[ol][q] = v4i{0, 0, 0, 0};
          if (sv) a[ol][q] = *reinterpret_cast<const v4i*>(gp + q * plane + at);
        }
      }
      const uint16_t* xb = xs + r16 * g.wxplane + r * g.SH * g.wxw + s8 * 8 * g.SW;
#pragma unroll
      for (int i = 0; i < kIdealTG; ++i) {
        if (i < tcount) {
          const uint16_t* xp = xb + toff[i];
          uint32_t wd[4];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            wd[e] = (uint32_t)xp[2 * e * g.SW] | ((uint32_t)xp[(2 * e + 1) * g.SW] << 16);
          const v8bf bx = as_v8bf(v4i{(int)wd[0], (int)wd[1], (int)wd[2], (int)wd[3]});
#pragma unroll
          for (int ol = 0; ol < kIdealOBG; ++ol)
#pragma unroll
            for (int q = 0; q < 3; ++q)
              acc[i][ol] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_v8bf(a[ol][q]), bx, acc[i][ol], 0, 0, 0);
        }
      }
    }
  }
  __syncthreads();
  v4f* red = reinterpret_cast<v4f*>(lds);
#pragma unroll
  for (int i = 0; i < kIdealTG; ++i)
#pragma unroll
    for (int ol = 0; ol < kIdealOBG; ++ol) red[((i * kIdealOBG + ol) * 4 + wave) * 64 + lane] = acc[i][ol];
  __syncthreads();
  for (int idx = tid; idx < kIdealTG * kIdealOBG * 64; idx += 256) {
    const int l = idx & 63, ai = idx >> 6;
    const int i = ai / kIdealOBG, ol = ai - i * kIdealOBG;
    const int ob = obp * kIdealOBG + ol;
    if (i >= tcount || ob >= g.nob) continue;
    v4f s = red[(ai * 4 + 0) * 64 + l];
    s += red[(ai * 4 + 1) * 64 + l];
    s += red[(ai * 4 + 2) * 64 + l];
    s += red[(ai * 4 + 3) * 64 + l];
    const int c = cb * 16 + (l & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = ob * 16 + 4 * (l >> 4) + r;
      slab[(((size_t)blockIdx.x * g.OP + o) * g.ntap + t0 + i) * g.Cp + c] = s[r];
    }
  }
}

// slabs in order -> grad_w (times sa, the weight STE mask) and one weight-LSQ partial per block
__global__ __launch_bounds__(256) void ideal_gw_finish_kernel(IdealG g, const float* __restrict__ w,
                                                              const float* __restrict__ slab,
                                                              const float* __restrict__ alpha_a,
                                                              const float* __restrict__ alpha_w,
                                                              float* __restrict__ gw, float* __restrict__ part_w) {
  __shared__ float red[4];
  const float sa = grad_scale_value(alpha_a[0], g.ga), sw = grad_scale_value(alpha_w[0], g.gw);
  const int n = g.O * g.C * g.ntap;
  const size_t sstride = (size_t)g.OP * g.ntap * g.Cp;
  float ps = 0.f;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
    const int t = e % g.ntap, oc = e / g.ntap;
    const int c = oc % g.C, o = oc / g.C;
    const size_t si = ((size_t)o * g.ntap + t) * g.Cp + c;
    float s = 0.f;
    for (int k = 0; k < g.wslabs; ++k) s += slab[k * sstride + si];
    const float dq = s * sa;  // d loss / d w_q
    const float tw = w[e] / sw;
    const bool inside = tw >= g.qn_w && tw <= g.qp_w;
    gw[e] = inside ? dq : 0.f;
    const float code = rintf(fminf(fmaxf(tw, g.qn_w), g.qp_w));
    ps += dq * (code - (inside ? tw : 0.f));
  }
  const float tot = ideal_block_sum(ps, red);
  if (threadIdx.x == 0) part_w[blockIdx.x] = tot;
}

// the two step-size gradients from their partials (one block, fixed order), grad_scale's factor applied
__global__ __launch_bounds__(256) void ideal_alpha_finish_kernel(IdealG g, int npa, const float* __restrict__ part_a,
                                                                 int npw, const float* __restrict__ part_w,
                                                                 float* __restrict__ ga_out,
                                                                 float* __restrict__ gw_out) {
  __shared__ float red[4];
  float a = 0.f, b = 0.f;
  for (int i = threadIdx.x; i < npa; i += blockDim.x) a += part_a[i];
  for (int i = threadIdx.x; i < npw; i += blockDim.x) b += part_w[i];
  const float ta = ideal_block_sum(a, red);
  __syncthreads();
  const float tb = ideal_block_sum(b, red);
  if (threadIdx.x == 0) {
    ga_out[0] = ta * g.ga;
    gw_out[0] = tb * g.gw;
  }
}

}  // namespace cimq
