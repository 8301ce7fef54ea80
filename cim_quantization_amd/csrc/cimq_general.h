// cimq_general.h -- the implicit-im2col tile machinery of the general kernels (cimq_kernels.hip,
// cimq_kernels_bwd.hip).
#pragma once
#include "cimq_device.h"

namespace cimq {

// =========================================================================================
// shared tile machinery: implicit im2col of the packed act codes into LDS
// =========================================================================================
// LDS image of one crossbar tile for 64 output pixels: As[j][row][KTP] int8 (row = pixel,
// contiguous f), built from the packed per-element codes; out-of-image taps are 0 (the
// zero padding of nn.Unfold).  Tables: foff[f] = c*H*W + kh*W + kw, fkk[f] = kh<<16|kw
// (-1 = beyond the tile), rowinfo[r] = {img base + ih0*W + iw0, ih0, iw0, valid}.
struct TileSmem {
  int8_t* As;     // [nba][64][KTP]
  int* foff;      // [KS*64]
  int* fkk;       // [KS*64]
  int4* rowinfo;  // [64]
};

__device__ inline void build_rowinfo(const Geo& g, int m0, int4* rowinfo) {
  const int t = threadIdx.x;
  if (t < 64) {
    const int m = m0 + t;
    int4 ri = make_int4(0, 0, 0, 0);
    if (m < g.M) {
      const int b = m / g.P, p = m - b * g.P;
      const int oh = p / g.Wo, ow = p - oh * g.Wo;
      const int ih0 = oh * g.SH - g.PH, iw0 = ow * g.SW - g.PW;
      ri = make_int4(b * g.C * g.HW + ih0 * g.W + iw0, ih0, iw0, 1);
    }
    rowinfo[t] = ri;
  }
}

__device__ inline void build_ftable(const Geo& g, int i, int* foff, int* fkk) {
  const int flo = i * g.xbar, flen = min(g.xbar, g.K - flo);
  for (int t = threadIdx.x; t < g.KS * 64; t += blockDim.x) {
    if (t < flen) {
      const int f = flo + t;
      const int c = f / g.KHW, rem = f - c * g.KHW;
      const int kh = rem / g.KW, kw = rem - kh * g.KW;
      foff[t] = c * g.HW + kh * g.W + kw;
      fkk[t] = (kh << 16) | kw;
    } else {
      foff[t] = 0;
      fkk[t] = -1;
    }
  }
}

// Gather one element's packed code (all slices) for pixel row r and tile column t.
template <int NBP>
__device__ inline uint2 gather_code(const Geo& g, const int8_t* __restrict__ xcode, const int4 ri,
                                    int fo, int fk) {
  uint2 c = make_uint2(0, 0);
  if (fk >= 0 && ri.w) {
    const int kh = fk >> 16, kw = fk & 0xFFFF;
    const int ih = ri.y + kh, iw = ri.z + kw;
    if (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W) {
      const long long idx = (long long)ri.x + fo;
      if (NBP == 4) c.x = reinterpret_cast<const uint32_t*>(xcode)[idx];
      else c = reinterpret_cast<const uint2*>(xcode)[idx];
    }
  }
  return c;
}

// Build As for the 64 pixels of rowinfo and tile (foff/fkk): each work item is 4
// consecutive tile columns of one pixel; the per-slice bytes are transposed into one
// dword per slice plane.
template <int NBP>
__device__ inline void build_As(const Geo& g, const int8_t* __restrict__ xcode, const TileSmem& sm) {
  const int quads = g.KS * 16;
  const int items = 64 * quads;
  for (int it = threadIdx.x; it < items; it += blockDim.x) {
    const int r = it / quads, q = it - r * quads;
    const int4 ri = sm.rowinfo[r];
    uint32_t pl[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int t = 4 * q + e;
      const uint2 c = gather_code<NBP>(g, xcode, ri, sm.foff[t], sm.fkk[t]);
#pragma unroll
      for (int j = 0; j < 4; ++j) pl[j] |= ((c.x >> (8 * j)) & 0xFFu) << (8 * e);
      if (NBP == 8) {
#pragma unroll
        for (int j = 0; j < 4; ++j) pl[4 + j] |= ((c.y >> (8 * j)) & 0xFFu) << (8 * e);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < g.nba) *reinterpret_cast<uint32_t*>(sm.As + ((size_t)j * 64 + r) * g.KTP + 4 * q) = pl[j];
  }
}

// Load the 16-byte MFMA operand of slice plane j for row (base16 + (lane&15)).
__device__ inline v4i load_xfrag(const Geo& g, const int8_t* As, int j, int row, int ks, int lane) {
  const int8_t* p = As + ((size_t)j * 64 + row) * g.KTP + ks * 64 + 16 * (lane >> 4);
  return *reinterpret_cast<const v4i*>(p);
}

}  // namespace cimq
