// cimq_prep.hip -- the prologue and reduction kernels of the Function entry points (cimq_api.hip): operands from
// a materialised x / w_q / alpha_q (cimq_operands.h), the slab sums, and the stand-alone LSQ activation backward.
#include "cimq_lsq_dev.h"
#include "cimq_operands.h"

namespace cimq {

// the slice words of every element of x (act_range)
__global__ void prep_act_kernel(Geo g, const float* __restrict__ x, const float* __restrict__ sa_p,
                                const float* __restrict__ signed_p, uint8_t* __restrict__ xcf,
                                uint8_t* __restrict__ xcb) {
  const float sa = *sa_p;
  const bool sgn = (*signed_p) != 0.f;
  act_range(g, x, sa, sgn, xcf, xcb, (long long)blockIdx.x * blockDim.x + threadIdx.x,
            (long long)gridDim.x * blockDim.x);
}
// the forward-only prologue (CIMQ_OPT_INFERENCE): the forward slice words alone
__global__ void prep_act_fwd_kernel(Geo g, const float* __restrict__ x, const float* __restrict__ sa_p,
                                    const float* __restrict__ signed_p, uint8_t* __restrict__ xcf) {
  const float sa = *sa_p;
  const bool sgn = (*signed_p) != 0.f;
  act_range<false>(g, x, sa, sgn, xcf, nullptr, (long long)blockIdx.x * blockDim.x + threadIdx.x,
                   (long long)gridDim.x * blockDim.x);
}

// the weight operands of the general / v3 forward (wfrag), the general grad_x (wgx) and the v8 grad_x (wcy)
__global__ void prep_wfrag_kernel(Geo g, const float* __restrict__ w_q, const float* __restrict__ sw_p,
                                  v4i* __restrict__ wfrag) {
  const WSrc ws{w_q, *sw_p, 0, 0.f, 0.f};
  const int total = g.T * g.KS * g.NBLK * WAVE;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x)
    wfrag_item(g, ws, wfrag, t);
}

__global__ void prep_wgx_kernel(Geo g, const float* __restrict__ w_q, const float* __restrict__ sw_p,
                                v4i* __restrict__ wgx) {
  const WSrc ws{w_q, *sw_p, 0, 0.f, 0.f};
  const int total = g.T * g.FBT * g.NKS * WAVE;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x)
    wgx_item(g, ws, wgx, t);
}

__global__ void prep_wcy_kernel(Geo g, const float* __restrict__ w_q, const float* __restrict__ sw_p, int ncpbt,
                                v4i* __restrict__ wcy) {
  const WSrc ws{w_q, *sw_p, 0, 0.f, 0.f};
  const int total = g.T * ncpbt * g.NKS * WAVE;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x)
    wcy_item(g, ws, ncpbt, wcy, t);
}

// ADC thresholds, STE intervals and mask coefficients (params_item)
__global__ void prep_params_kernel(Geo g, const float* __restrict__ alpha_q, const float* __restrict__ sw_p,
                                   const float* __restrict__ sa_p, const int8_t* __restrict__ bmask,
                                   Params pp, const float* __restrict__ beta) {
  const float sw = *sw_p, sa = *sa_p;
  const ASrc as{alpha_q, 0, 0.f, 0.f};
  const int total = g.T * g.nba * g.nbw * g.Opad + g.nbw * g.nba + (beta != nullptr ? g.Opad : 0);
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x)
    if (params_item(g, as, sw, sa, bmask, pp, t, beta)) pp.flags[0] = 1;  // every writer stores 1
}

// grad_w and grad_alpha (or the alpha_cim init value) from the per-chunk slabs, summed in chunk order
__global__ __launch_bounds__(1024) void reduce_gw_v3_kernel(Geo g, int nchunks, const float* __restrict__ gw_slab,
                                                            const float* __restrict__ sa_p,
                                                            float* __restrict__ grad_w) {
  __shared__ float red[1024];
  const size_t rows = (size_t)g.T * g.FBT * 16;  // (tile, f-in-tile)
  const size_t nout = rows * g.Opad;
  const size_t idx = (size_t)blockIdx.x * 64 + (threadIdx.x & 63);
  const float v = reduce_chunks(gw_slab, nout, nchunks, idx < nout ? idx : 0, red);
  if ((threadIdx.x >> 6) == 0 && idx < nout) {
    const int o = (int)(idx % g.Opad);
    const size_t row = idx / g.Opad;
    const int i = (int)(row / (g.FBT * 16)), fl = (int)(row - (size_t)i * g.FBT * 16);
    const int f = i * g.xbar + fl;
    if (o < g.O && fl < g.xbar && f < g.K) grad_w[(size_t)o * g.K + f] = v * ((*sa_p) / (float)g.nbw);
  }
}

__global__ __launch_bounds__(1024) void reduce_galpha_v3_kernel(Geo g, int nchunks, const float* __restrict__ ga_slab,
                                                                Params pp, float cgrad, int init,
                                                                const float* __restrict__ sw_p,
                                                                const float* __restrict__ sa_p, float count,
                                                                float sqrt_qp, float* __restrict__ out) {
  __shared__ float red[1024];
  const int nkj = g.nbw * g.nba;
  const size_t nout = (size_t)g.T * nkj * g.Opad;
  const size_t idx = (size_t)blockIdx.x * 64 + (threadIdx.x & 63);
  const float s = reduce_chunks(ga_slab, nout, nchunks, idx < nout ? idx : 0, red);
  if ((threadIdx.x >> 6) == 0 && idx < nout) {
    const int o = (int)(idx % g.Opad);
    const size_t q = idx / g.Opad;  // (i, k, j)
    if (o < g.O) {
      const int kj = (int)(q % nkj);
      const int i = (int)(q / nkj);
      const int k = kj / g.nba, j = kj - k * g.nba;
      const size_t dst = (((size_t)i * g.nbw + k) * g.nba + j) * g.O + o;  // [1,T,nbw,nba,1,O]
      if (init) {
        const float mean = s / count;
        const float v = (2.0f * mean) / sqrt_qp;
        out[dst] = (v == 0.f) ? (1.0f * (*sw_p)) * (*sa_p) : v;  // lsq.py:560-561
      } else {
        out[dst] = (cgrad * pp.ckj[kj]) * s;
      }
    }
  }
}

// =========================================================================================
// LSQ activation quantiser backward (autograd of lsq.py:547-549, fused-module path)
// =========================================================================================
//   y1 = x/sa ; c = clamp(y1,0,Qp) ; x_q = round_pass(c)*sa
//   g_y1 = (0<=y1<=Qp) ? g*sa : 0 ;  g_x = g_y1/sa
//   g_sa = sum(g*round(c)) + sum(-g_y1*((x/sa)/sa))
__global__ void lsq_act_bwd_kernel(long long n, const float* __restrict__ x, const float* __restrict__ sa_p,
                                   float qp, float* __restrict__ gx_inout, float* __restrict__ partial) {
  __shared__ float sred[256];
  const float sa = *sa_p;
  float acc = 0.f;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < n;
       idx += (long long)gridDim.x * blockDim.x) {
    const float xv = x[idx];
    const float gq = gx_inout[idx];
    const float y1 = xv / sa;
    const float c = clamp_nan(y1, 0.f, qp);
    const float r = rintf(c);
    const float rp = (r - c) + c;
    const bool pass = (y1 >= 0.f) && (y1 <= qp);
    const float gy = pass ? gq * sa : 0.f;
    gx_inout[idx] = gy / sa;
    acc += gq * rp;
    acc += -(gy * (y1 / sa));
  }
  sred[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sred[threadIdx.x] += sred[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = sred[0];
}

__global__ void sum_partials_kernel(int n, const float* __restrict__ partial, float* __restrict__ out) {
  __shared__ float sred[256];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) acc += partial[i];
  sred[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sred[threadIdx.x] += sred[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sred[0];
}

}  // namespace cimq
