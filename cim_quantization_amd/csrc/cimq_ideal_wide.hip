// cimq_ideal_wide.hip -- the ideal-ADC conv's backward for its large layers (ideal_wide_plan, CIMQ_OPT_WIDE_BWD):
// 3 x 3, stride 1, pad 1, W in {8, 16, 32}, C >= 128, C % 16 == 0, O % 32 == 0.  A 64-pixel tile is 64 / W whole rows
// of one image, so every tap is a constant offset into a patch with a zero halo and no lane evaluates a predicate:
//   grad_x: grad_out (hi / mid / lo bf16) as [row + halo][col + halo][o] in LDS is the MFMA's A operand, one aligned
//           ds_read_b128 per plane at pixel base + tap offset; the weight-code fragments of ideal_prep_w_kernel are B,
//           straight from global memory, the next k-step's loaded ahead of this one's MFMAs
//   grad_w: the activation codes are staged three times, pre-shifted by kw, so the B operand of tap (kh, kw) is one
//           aligned ds_read_b128 at a row offset; a wave keeps two output blocks x one input block x nine taps in
//           registers over all stages of its slab: no split of k across waves, no reduction in LDS
// Three v_mfma_f32_16x16x32_bf16 per product as in cimq_ideal.hip, no atomics, every sum in a fixed order.
// Included by cimq_part_ideal_wide.hip; the slabs and partials feed ideal_gw_finish_kernel / ideal_alpha_finish_kernel.
#pragma once
#include "cimq_ideal_dev.h"

namespace cimq {

__device__ inline uint32_t ideal_code_pk(float a, float b, float sa, float qp) {  // two codes as bf16 (exact), low a
  return (__float_as_uint(ideal_code(a, sa, 0.f, qp)) >> 16) | (__float_as_uint(ideal_code(b, sa, 0.f, qp)) & 0xffff0000u);
}

// ---------------------------------------------------------------------------------------
// grad_x.  Workgroup = one 64-pixel whole-row tile of one image (blockIdx.x) x kIdealWideCB input-channel blocks
// (blockIdx.y); wave w owns pixels 16 w .. 16 w + 15 and all of the blocks.  Per output-channel chunk the grad_out rows
// the tile meets are staged once (two channels x four pixels per item, float4 reads); rows outside the image and the
// halo columns stay zero from the start.  D[pixel][c]: a lane holds four consecutive pixels of one channel, so the
// epilogue (times sw, the clamp mask, the act-LSQ partial) reads x and writes grad_x as float4.  LDS: hi | mid | lo.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cim_ideal_gx_wide_kernel(IdealG g, IdealWideG v, const float* __restrict__ x,
                                                                const float* __restrict__ gout,
                                                                const v4i* __restrict__ wx,
                                                                const float* __restrict__ alpha_a,
                                                                const float* __restrict__ alpha_w,
                                                                float* __restrict__ gx, float* __restrict__ part_a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, g4 = lane >> 4;
  const int b = blockIdx.x / v.mt, t = blockIdx.x - b * v.mt;
  const int oh0 = t * v.rows, p0 = t * 64;
  const int cb0 = blockIdx.y * kIdealWideCB;
  const int pw = g.W + 2, qrow = g.W >> 2;
  for (int i = tid; i < 3 * (v.xplane >> 4); i += 256) reinterpret_cast<v4i*>(lds)[i] = v4i{0, 0, 0, 0};
  // patch rows pr_lo .. pr_lo + nrs - 1 are in the image (patch row pr is grad_out row oh0 - 1 + pr)
  const int pr_lo = oh0 == 0 ? 1 : 0;
  const int nrs = (oh0 + v.rows == g.H ? v.rows : v.rows + 1) - pr_lo + 1;
  const int nq = nrs * qrow, items = (g.noc >> 1) * nq;
  const int pix = wave * 16 + r16;
  const int lr = pix / g.W, iw = pix - lr * g.W;
  const uint8_t* abase = lds + (lr * pw + iw) * v.xpitch + g4 * 16;
  const v4i* wb[kIdealWideCB];
#pragma unroll
  for (int i = 0; i < kIdealWideCB; ++i)  // (a block past the last reads the last one's fragments: in bounds, not stored)
    wb[i] = wx + (size_t)min(cb0 + i, g.ncb - 1) * v.xsteps * 64 + lane;
  v4i cur[kIdealWideCB], nxt[kIdealWideCB];
  v4f acc[kIdealWideCB];
#pragma unroll
  for (int i = 0; i < kIdealWideCB; ++i) {
    cur[i] = wb[i][0];
    acc[i] = v4f{0.f, 0.f, 0.f, 0.f};
  }
  int kk = 0;  // the k-step over all chunks: the fragments of one block are contiguous in (chunk, k-step)
  for (int och = 0; och < g.xnoch; ++och) {
    __syncthreads();  // the zero fill / the previous chunk's reads
    for (int it = tid; it < items; it += 256) {
      const int rest = it >> 3;
      const int q = rest % nq, o2 = (rest / nq) * 8 + (it & 7);
      const int o = och * g.noc + o2 * 2;
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), c = a;
      if (o < g.O) {  // (O is even: o + 1 < O too)
        const size_t gi = ((size_t)b * g.O + o) * g.P + (size_t)(oh0 - 1 + pr_lo) * g.W + q * 4;
        a = *reinterpret_cast<const float4*>(gout + gi);
        c = *reinterpret_cast<const float4*>(gout + gi + g.P);
      }
      const int prow = pr_lo + q / qrow, col = (q % qrow) * 4;
      uint8_t* at = lds + ((prow * pw + col + 1) * v.xpitch + o2 * 4);
      const float av[4] = {a.x, a.y, a.z, a.w}, cv[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t hi, mid, lo;
        split3_pk(av[j], cv[j], hi, mid, lo);
        *reinterpret_cast<uint32_t*>(at + j * v.xpitch) = hi;
        *reinterpret_cast<uint32_t*>(at + j * v.xpitch + v.xplane) = mid;
        *reinterpret_cast<uint32_t*>(at + j * v.xpitch + 2 * v.xplane) = lo;
      }
    }
    __syncthreads();
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const uint8_t* ap = abase + ((2 - tap / 3) * pw + (2 - tap % 3)) * v.xpitch;
      for (int og = 0; og < v.nog; ++og) {
        const int nk = min(kk + 1, v.xsteps - 1);
#pragma unroll
        for (int i = 0; i < kIdealWideCB; ++i) nxt[i] = wb[i][(size_t)nk * 64];
        const v8bf ah = as_v8bf(*reinterpret_cast<const v4i*>(ap + og * 64));
        const v8bf am = as_v8bf(*reinterpret_cast<const v4i*>(ap + og * 64 + v.xplane));
        const v8bf al = as_v8bf(*reinterpret_cast<const v4i*>(ap + og * 64 + 2 * v.xplane));
#pragma unroll
        for (int i = 0; i < kIdealWideCB; ++i) {
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, as_v8bf(cur[i]), acc[i], 0, 0, 0);
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, as_v8bf(cur[i]), acc[i], 0, 0, 0);
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, as_v8bf(cur[i]), acc[i], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < kIdealWideCB; ++i) cur[i] = nxt[i];
        ++kk;
      }
    }
  }
  const float sa = grad_scale_value(alpha_a[0], g.ga), sw = grad_scale_value(alpha_w[0], g.gw);
  float ps = 0.f;
#pragma unroll
  for (int i = 0; i < kIdealWideCB; ++i) {
    if (cb0 + i >= g.ncb) continue;
    const size_t xi = ((size_t)b * g.C + (cb0 + i) * 16 + r16) * g.P + p0 + wave * 16 + 4 * g4;
    const float4 xv4 = *reinterpret_cast<const float4*>(x + xi);
    const float xv[4] = {xv4.x, xv4.y, xv4.z, xv4.w};
    float o4[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float tq = xv[r] / sa;
      const bool inside = tq >= 0.f && tq <= g.qp_a;
      const float dq = acc[i][r] * sw;  // d loss / d x_q
      o4[r] = inside ? dq : 0.f;
      const float code = rintf(fminf(fmaxf(tq, 0.f), g.qp_a));
      ps += dq * (code - (inside ? tq : 0.f));
    }
    *reinterpret_cast<float4*>(gx + xi) = make_float4(o4[0], o4[1], o4[2], o4[3]);
  }
  const float tot = ideal_block_sum(ps, red);
  if (tid == 0) part_a[blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

// ---------------------------------------------------------------------------------------
// grad_w.  Workgroup = slab (blockIdx.x: wspc 64-pixel whole-row stages) x 32 input channels (blockIdx.y) x 64 output
// channels (blockIdx.z); wave (wo, wc) owns output blocks 2 wo, 2 wo + 1, input block wc and all nine taps.  Per stage:
// grad_out as three bf16 planes [o][pixel] (kIdealWideGPitch bytes an o) and the rows of x the stage meets, requantised
// with the forward's own division, as planes [kw][c][row + halo][ow] holding the code of column ow + kw - 1 (zero off
// the image); a thread's share of the next stage is in registers while the MFMAs of this one run.  A k-step is 32
// pixels, four 8-pixel segments of whole rows: 6 A reads and 9 B reads for 54 MFMAs.  LDS: codes | hi | mid | lo.
// ---------------------------------------------------------------------------------------
struct IdealWideStage {
  float4 gr[2][2];  // grad_out: two items of 8 pixels
  float4 xr[2][2];  // x: two items of 8 pixels ...
  float xl[2], xe[2];  // ... and the pixel left and right of each
};

__device__ inline void ideal_wide_load(const IdealG& g, const IdealWideG& v, const float* __restrict__ x,
                                       const float* __restrict__ gout, int u, int c0, int o0, IdealWideStage& s) {
  const int b = u / v.mt, t = u - b * v.mt;
  const int tid = threadIdx.x, s8n = g.W >> 3;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int it = tid + 256 * j;
    const int o = o0 + (it >> 3);
    s.gr[j][0] = s.gr[j][1] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (o < g.O) {
      const float4* p = reinterpret_cast<const float4*>(gout + ((size_t)b * g.O + o) * g.P + t * 64 + (it & 7) * 8);
      s.gr[j][0] = p[0];
      s.gr[j][1] = p[1];
    }
    const int s8 = it % s8n, rest = it / s8n;
    const int prow = rest % (v.rows + 2), c = c0 + rest / (v.rows + 2);
    const int ih = t * v.rows - 1 + prow;
    s.xr[j][0] = s.xr[j][1] = make_float4(0.f, 0.f, 0.f, 0.f);
    s.xl[j] = s.xe[j] = 0.f;
    if (it < v.wnxi && c < g.C && ih >= 0 && ih < g.H) {
      const float* xp = x + (((size_t)b * g.C + c) * g.H + ih) * g.W + s8 * 8;
      s.xr[j][0] = reinterpret_cast<const float4*>(xp)[0];
      s.xr[j][1] = reinterpret_cast<const float4*>(xp)[1];
      if (s8 > 0) s.xl[j] = xp[-1];
      if (s8 < s8n - 1) s.xe[j] = xp[8];
    }
  }
}

__device__ inline void ideal_wide_store(const IdealG& g, const IdealWideG& v, float sa, const IdealWideStage& s,
                                        uint8_t* codes, uint8_t* gp) {
  const int tid = threadIdx.x, s8n = g.W >> 3;
  const int gplane = 64 * kIdealWideGPitch, kwplane = 32 * v.wcpitch;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int it = tid + 256 * j;
    const float gv[8] = {s.gr[j][0].x, s.gr[j][0].y, s.gr[j][0].z, s.gr[j][0].w,
                         s.gr[j][1].x, s.gr[j][1].y, s.gr[j][1].z, s.gr[j][1].w};
    uint32_t hi[4], mid[4], lo[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) split3_pk(gv[2 * e], gv[2 * e + 1], hi[e], mid[e], lo[e]);
    uint8_t* at = gp + (it >> 3) * kIdealWideGPitch + (it & 7) * 16;
    *reinterpret_cast<v4i*>(at) = v4i{(int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
    *reinterpret_cast<v4i*>(at + gplane) = v4i{(int)mid[0], (int)mid[1], (int)mid[2], (int)mid[3]};
    *reinterpret_cast<v4i*>(at + 2 * gplane) = v4i{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3]};
    if (it < v.wnxi) {
      const int s8 = it % s8n, rest = it / s8n;
      const int prow = rest % (v.rows + 2), cl = rest / (v.rows + 2);
      // (a zero stands for every pixel off the image or past C: its code is 0)
      const float xv[10] = {s.xl[j],      s.xr[j][0].x, s.xr[j][0].y, s.xr[j][0].z, s.xr[j][0].w,
                            s.xr[j][1].x, s.xr[j][1].y, s.xr[j][1].z, s.xr[j][1].w, s.xe[j]};
      uint32_t ev[5], od[4];  // codes (0,1) (2,3) .. (8,9) and (1,2) .. (7,8)
#pragma unroll
      for (int e = 0; e < 5; ++e) ev[e] = ideal_code_pk(xv[2 * e], xv[2 * e + 1], sa, g.qp_a);
#pragma unroll
      for (int e = 0; e < 4; ++e) od[e] = (ev[e] >> 16) | (ev[e + 1] << 16);
      uint8_t* ct = codes + cl * v.wcpitch + (prow * g.W + s8 * 8) * 2;
      *reinterpret_cast<v4i*>(ct) = v4i{(int)ev[0], (int)ev[1], (int)ev[2], (int)ev[3]};               // kw 0: ow - 1
      *reinterpret_cast<v4i*>(ct + kwplane) = v4i{(int)od[0], (int)od[1], (int)od[2], (int)od[3]};     // kw 1: ow
      *reinterpret_cast<v4i*>(ct + 2 * kwplane) = v4i{(int)ev[1], (int)ev[2], (int)ev[3], (int)ev[4]};  // kw 2: ow + 1
    }
  }
}

__global__ __launch_bounds__(256) void cim_ideal_gw_wide_kernel(IdealG g, IdealWideG v, const float* __restrict__ x,
                                                                const float* __restrict__ gout,
                                                                const float* __restrict__ alpha_a,
                                                                float* __restrict__ slab) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int kwplane = 32 * v.wcpitch, gplane = 64 * kIdealWideGPitch;
  uint8_t* codes = lds;
  uint8_t* gp = lds + 3 * kwplane;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, g4 = lane >> 4;
  const int wo = wave >> 1, wc = wave & 1;
  const int c0 = blockIdx.y * 32, o0 = blockIdx.z * 64;
  const bool act = c0 + wc * 16 < g.C && o0 + wo * 32 < g.O;  // (wave-uniform; C % 16 == 0 and O % 32 == 0)
  const float sa = grad_scale_value(alpha_a[0], g.ga);
  v4f acc[2][9];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) acc[j][tap] = v4f{0.f, 0.f, 0.f, 0.f};
  const int u0 = blockIdx.x * v.wspc, u1 = min(v.wunits, u0 + v.wspc);
  IdealWideStage st;
  ideal_wide_load(g, v, x, gout, u0, c0, o0, st);
  for (int u = u0; u < u1; ++u) {
    __syncthreads();  // the previous stage's reads
    ideal_wide_store(g, v, sa, st, codes, gp);
    __syncthreads();
    if (u + 1 < u1) ideal_wide_load(g, v, x, gout, u + 1, c0, o0, st);
    if (!act) continue;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int seg = ks * 4 + g4;
      const int lr = (seg * 8) / g.W, ow0 = seg * 8 - lr * g.W;
      v8bf a[2][3];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 3; ++q)
          a[j][q] = as_v8bf(*reinterpret_cast<const v4i*>(gp + q * gplane +
                                                          ((wo * 2 + j) * 16 + r16) * kIdealWideGPitch + seg * 16));
      const uint8_t* cp = codes + (wc * 16 + r16) * v.wcpitch + (lr * g.W + ow0) * 2;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const v8bf bx = as_v8bf(*reinterpret_cast<const v4i*>(cp + (tap % 3) * kwplane + (tap / 3) * g.W * 2));
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int q = 0; q < 3; ++q)
            acc[j][tap] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[j][q], bx, acc[j][tap], 0, 0, 0);
      }
    }
  }
  if (!act) return;
  const int c = c0 + wc * 16 + r16;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = o0 + (wo * 2 + j) * 16 + 4 * g4 + r;
        slab[(((size_t)blockIdx.x * g.OP + o) * 9 + tap) * g.Cp + c] = acc[j][tap][r];
      }
}

}  // namespace cimq
