// cimq_c1w.hip -- the backward of a w8a8 first conv with O = 16 n output channels, n >= 2, chosen under
// CIMQ_OPT_WIDE_BWD where c1w_plan holds (CIMQ_ROUTE_C1W): cim_bwd_c1_kernel<true, true>, the multi-output-block
// instance of the first conv's recompute kernel (cimq_c1.hip: how the blocks are walked and grad_x summed over them
// is described there), and c1w_fold_kernel, which adds the grad_x partials of an image's output-block groups where
// there are several.
#include "cimq_c1.hip"

namespace cimq {

// the name the route's kernel goes by (traces show the instance, cim_bwd_c1_kernel<true, true>)
constexpr auto cim_bwd_c1w_kernel = cim_bwd_c1_kernel<true, true>;

// Several groups: grad_x of image b = the group partials added in ascending order, times sw / nba, through the
// act-LSQ backward; one d loss / d sa partial per workgroup (WsLayout::lsq_part)
__global__ __launch_bounds__(256) void c1w_fold_kernel(Geo g, int groups, const float* __restrict__ part,
                                                       const float* __restrict__ sw_p, const float* __restrict__ sa_p,
                                                       const float* __restrict__ x, float* __restrict__ gx,
                                                       float* __restrict__ gsa_part) {
  __shared__ float apart[4];
  const int b = (int)blockIdx.x;
  const int n4 = g.C * g.HW / 4;  // (W % 8 == 0: c1w_plan)
  const float sa = *sa_p, scale = *sw_p / 8.f, inv_sa = 1.f / sa;
  const size_t base = (size_t)b * g.C * g.HW;
  float gsum = 0.f;
  for (int t = threadIdx.x; t < n4; t += blockDim.x) {
    const size_t gi = base + (size_t)t * 4;
    float4 a = *reinterpret_cast<const float4*>(part + gi);
    for (int q = 1; q < groups; ++q) {
      const float4 p = *reinterpret_cast<const float4*>(part + (size_t)q * (size_t)g.Nin + gi);
      a.x += p.x; a.y += p.y; a.z += p.z; a.w += p.w;
    }
    const float4 xv = *reinterpret_cast<const float4*>(x + gi);
    float4 o;
    o.x = c1_act_lsq(a.x, scale, xv.x, sa, inv_sa, g.lsq_qp, &gsum);
    o.y = c1_act_lsq(a.y, scale, xv.y, sa, inv_sa, g.lsq_qp, &gsum);
    o.z = c1_act_lsq(a.z, scale, xv.z, sa, inv_sa, g.lsq_qp, &gsum);
    o.w = c1_act_lsq(a.w, scale, xv.w, sa, inv_sa, g.lsq_qp, &gsum);
    *reinterpret_cast<float4*>(gx + gi) = o;
  }
  for (int o = 32; o > 0; o >>= 1) gsum += __shfl_xor(gsum, o);
  if ((threadIdx.x & 63) == 0) apart[threadIdx.x >> 6] = gsum;
  __syncthreads();
  if (threadIdx.x == 0) gsa_part[b] = ((apart[0] + apart[1]) + apart[2]) + apart[3];
}

}  // namespace cimq
