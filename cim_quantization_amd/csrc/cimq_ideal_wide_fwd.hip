// cimq_ideal_wide_fwd.hip -- the ideal-ADC conv's forward for its large layers (ideal_wide_fwd_plan, CIMQ_OPT_WIDE_BWD):
// 3 x 3, stride 1, pad 1, W in {8, 16, 32}, C >= 128, C % 16 == 0, O % 32 == 0, bits_a <= 7.  A 64-pixel tile is
// 64 / W whole rows of one image, so the patch [row + halo][col + halo][channel] (bytes, ideal_plan's fpitch) has a
// zero halo, every tap is a constant offset and no lane evaluates a predicate:
//   staging : x as float4 (four pixels of one channel), four channels an item, quantised with the forward's own IEEE
//             division, transposed in registers and written as four 32-bit words (four channels of one pixel); once per
//             workgroup where the channels fit one chunk, the patch then serves every output group of the workgroup
//   k-step  : PB ds_read_b128 of the patch (the MFMA's A operand: 16 pixels x 16 channels of one tap per lane group)
//             against four wf fragments of ideal_prep_w_kernel (B, one contiguous 4 KB run of global memory), the next
//             k-step's fragments and tap offsets loaded before this one's 4 PB v_mfma_i32_16x16x64_i8
//   store   : D[pixel][o]: a lane holds four consecutive pixels of one output channel, one float4
// The int32 sum is exact and the scaling is cim_ideal_fwd_kernel's expression, so out is that kernel's bit for bit.
// No atomics.  Included by cimq_part_ideal_wide_fwd.hip.
#pragma once
#include "cimq_ideal_dev.h"

namespace cimq {

// One chunk's in-image rows and columns into the patch.  Item = (four channels c4, four pixels q of one row); the 16
// low lane bits walk c4, the next two walk q: a wave's store is four runs of 16 consecutive words whose starts lie
// 4 * fpitch bytes = 16 * odd words apart -- every bank once; where the four q of a wave wrap to the next row (W = 8)
// two runs overlap: a two-way conflict at most.
__device__ inline void ideal_wide_fwd_stage(const IdealG& g, const float* __restrict__ x, uint8_t* patch, int b, int ch,
                                            int oh0, int pr_lo, int nrs, float sa) {
  const int qrow = g.W >> 2, nq = nrs * qrow;
  const int nc4 = g.ncx >> 2;
  const int items = ((nc4 + 15) >> 4) * nq * 16;
  for (int it = threadIdx.x; it < items; it += 256) {
    const int rest = it >> 4;
    const int q = rest % nq, c4 = (rest / nq) * 16 + (it & 15);
    if (c4 >= nc4) continue;
    const int prow = pr_lo + q / qrow, col = (q % qrow) * 4;
    const int c = ch * g.ncx + c4 * 4;
    uint32_t wd[4] = {0u, 0u, 0u, 0u};  // (channels past C -- the last chunk's tail -- are zero codes; C % 4 == 0)
    if (c < g.C) {
      const float* xp = x + (((size_t)b * g.C + c) * g.H + (oh0 - 1 + prow)) * g.W + col;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 f = *reinterpret_cast<const float4*>(xp + (size_t)j * g.P);
        wd[0] |= ((uint32_t)(int)ideal_code(f.x, sa, 0.f, g.qp_a)) << (8 * j);
        wd[1] |= ((uint32_t)(int)ideal_code(f.y, sa, 0.f, g.qp_a)) << (8 * j);
        wd[2] |= ((uint32_t)(int)ideal_code(f.z, sa, 0.f, g.qp_a)) << (8 * j);
        wd[3] |= ((uint32_t)(int)ideal_code(f.w, sa, 0.f, g.qp_a)) << (8 * j);
      }
    }
    uint8_t* at = patch + (size_t)(prow * g.fwp + col + 1) * g.fpitch + c4 * 4;
#pragma unroll
    for (int p = 0; p < 4; ++p) *reinterpret_cast<uint32_t*>(at + p * g.fpitch) = wd[p];
  }
}

// ---------------------------------------------------------------------------------------
// Workgroup = one 64-pixel whole-row tile of one image (blockIdx.x) x gpw output groups of 4 PB output blocks
// (blockIdx.y).  Wave (wp, wo) owns pixel blocks wp PB .. wp PB + PB - 1 and output blocks 4 wo .. 4 wo + 3 of each
// group: PB x 4 accumulators, alive across the channel chunks of a group.  With one chunk the patch is staged once and
// stays for all groups; with more it is restaged per (group, chunk) -- only in-image rows and columns are written, so
// the halo stays zero from the one fill.  A fragment's k beyond the contraction is zero (ideal_prep_w_kernel), so its
// lanes read offset 0 of the patch.  LDS: tap table [fks * 4] ints | patch (ideal_plan's flds).
// ---------------------------------------------------------------------------------------
template <int PB>
__global__ __launch_bounds__(256) void cim_ideal_fwd_wide_kernel(IdealG g, IdealWideFwdG v,
                                                                 const float* __restrict__ x,
                                                                 const v4i* __restrict__ wf,
                                                                 const float* __restrict__ alpha_a,
                                                                 const float* __restrict__ alpha_w,
                                                                 float* __restrict__ out) {
  constexpr int OB = kIdealWideFwdOB, PWV = 4 / PB;  // waves along the pixels
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  int* tab = reinterpret_cast<int*>(lds);
  uint8_t* patch = lds + g.fks * 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, g4 = lane >> 4;
  const int wp = wave % PWV, wo = wave / PWV;
  const int b = blockIdx.x / v.mt, t = blockIdx.x - b * v.mt;
  const int oh0 = t * v.rows, p0 = t * 64;
  const float sa = grad_scale_value(alpha_a[0], g.ga);
  for (int i = tid; i < (g.frows * g.fwp * g.fpitch) >> 4; i += 256) reinterpret_cast<v4i*>(patch)[i] = v4i{0, 0, 0, 0};
  const int g16 = g.ncx >> 4;
  for (int kc = tid; kc < g.fks * 4; kc += 256) {
    const int tap = kc / g16, cg = kc - tap * g16;
    tab[kc] = tap < 9 ? ((tap / 3) * g.fwp + tap % 3) * g.fpitch + cg * 16 : 0;
  }
  // patch rows pr_lo .. pr_lo + nrs - 1 are in the image (patch row pr is input row oh0 - 1 + pr)
  const int pr_lo = oh0 == 0 ? 1 : 0;
  const int nrs = (oh0 + v.rows == g.H ? v.rows : v.rows + 1) - pr_lo + 1;
  const uint8_t* abase[PB];
#pragma unroll
  for (int p = 0; p < PB; ++p) {
    const int pix = (wp * PB + p) * 16 + r16;
    const int lr = pix / g.W, iw = pix - lr * g.W;
    abase[p] = patch + (lr * g.fwp + iw) * g.fpitch;
  }
  const float sw = grad_scale_value(alpha_w[0], g.gw);
  for (int gi = 0; gi < v.gpw; ++gi) {
    const int og = blockIdx.y * v.gpw + gi;
    if (og >= v.ngroups) break;  // (the same for the whole workgroup)
    const int ob0 = og * (PB * OB) + wo * OB;
    int obi[OB];  // (a block past the last reads the last one's fragments: in bounds, not stored)
#pragma unroll
    for (int i = 0; i < OB; ++i) obi[i] = min(ob0 + i, g.nob - 1) * 64 + lane;
    v4i acc[PB][OB];
#pragma unroll
    for (int p = 0; p < PB; ++p)
#pragma unroll
      for (int i = 0; i < OB; ++i) acc[p][i] = v4i{0, 0, 0, 0};
    for (int ch = 0; ch < g.nch; ++ch) {
      if (g.nch > 1 || gi == 0) {
        __syncthreads();  // the zero fill and the table / the previous chunk's reads
        ideal_wide_fwd_stage(g, x, patch, b, ch, oh0, pr_lo, nrs, sa);
        __syncthreads();
      }
      if (ob0 >= g.nob) continue;  // (wave-uniform: a tail group narrower than the workgroup's span)
      const v4i* wfc = wf + (size_t)ch * g.fks * g.nob * 64;
      v4i cur[OB], nxt[OB];
#pragma unroll
      for (int i = 0; i < OB; ++i) cur[i] = wfc[obi[i]];
      int off = tab[g4];
      for (int ks = 0; ks < g.fks; ++ks) {
        const int nk = min(ks + 1, g.fks - 1);
#pragma unroll
        for (int i = 0; i < OB; ++i) nxt[i] = wfc[(size_t)nk * g.nob * 64 + obi[i]];
        const int noff = tab[nk * 4 + g4];
        v4i a[PB];
#pragma unroll
        for (int p = 0; p < PB; ++p) a[p] = *reinterpret_cast<const v4i*>(abase[p] + off);
#pragma unroll
        for (int p = 0; p < PB; ++p)
#pragma unroll
          for (int i = 0; i < OB; ++i) acc[p][i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[p], cur[i], acc[p][i], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < OB; ++i) cur[i] = nxt[i];
        off = noff;
      }
    }
#pragma unroll
    for (int i = 0; i < OB; ++i) {
      if (ob0 + i >= g.nob) continue;
      float* op = out + ((size_t)b * g.O + (ob0 + i) * 16 + r16) * g.P + p0 + wp * PB * 16 + 4 * g4;
#pragma unroll
      for (int p = 0; p < PB; ++p)
        *reinterpret_cast<float4*>(op + p * 16) =
            make_float4(((float)acc[p][i][0] * sa) * sw, ((float)acc[p][i][1] * sa) * sw,
                        ((float)acc[p][i][2] * sa) * sw, ((float)acc[p][i][3] * sa) * sw);
    }
  }
}

}  // namespace cimq
