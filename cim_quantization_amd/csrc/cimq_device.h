// cimq_device.h -- geometry, parameter tables and exact-fp32 device helpers shared by the
// libcimq kernels.  Compiled only for gfx950 (CDNA4): 64-lane waves, MFMA int8/bf16.
#pragma once

#include <hip/hip_fp16.h>

// every kernel's lane math (16-lane MFMA rows, xor-32 butterflies, threadIdx >> 6 wave ids)
// assumes 64-lane wavefronts (CDNA)
#if defined(__HIP_DEVICE_COMPILE__) && defined(__AMDGCN_WAVEFRONT_SIZE) && __AMDGCN_WAVEFRONT_SIZE != 64
#error "libcimq assumes 64-lane wavefronts (gfx9 CDNA targets)"
#endif
#include "cimq_types.h"

// The kernels assume 64-lane waves (shuffle butterflies over 32..1, threadIdx >> 6 as the
// wave id): build.py accepts only gfx9 (wave64-only) targets.
namespace cimq {

// ---------------------------------------------------------------------------------------
// exact fp32 emulation of the reference's torch op sequence (compiled with -ffp-contract=off)
// ---------------------------------------------------------------------------------------
__device__ inline float pow2f(int e) { return __int_as_float((127 + e) << 23); }  // |e| < 127

// torch.remainder(t, 2^bs) for float t: floor-mod, result has the divisor's sign.
__device__ inline float rem_pow2(float t, int bs) {
  const float b = (float)(1 << bs);
  return t - b * floorf(t * pow2f(-bs));
}

// Plane k of the reference's slicing of a non-negative magnitude v (lsq.py:454-457 / 475-478):
// floor(v / (2^bs)^k) for k >= 1, then remainder 2^bs.
__device__ inline float slice_mag(float v, int k, int bs) {
  float t = (k == 0) ? v : floorf(v * pow2f(-bs * k));
  return rem_pow2(t, bs);
}

// slicing_act (unsigned, lsq.py:466-480): the same digit extraction on the raw value.
__device__ inline float slice_unsigned(float v, int k, int bs) { return slice_mag(v, k, bs); }

// slicing_weights_signed / slicing_act_signed (lsq.py:438-464, 483-509): slice the positive
// part and the negated negative part separately and subtract.
__device__ inline float slice_signed(float v, int k, int bs) {
  float pos = (v <= 0.f) ? 0.f : v;
  float neg = (v >= 0.f) ? 0.f : v;
  neg = -1.f * neg;
  return slice_mag(pos, k, bs) - slice_mag(neg, k, bs);
}

// The output epilogue (Epi) on a value about to be stored: v * scale, + shift, + residual, ReLU, each one IEEE
// fp32 operation in that order (what torch's mul, add, add, relu give on the stored tensor; a NaN stays NaN).
// sc / sh are the lane's channel entries, read once by the caller; rv is read at the store's own address.
__device__ inline float epi_val(float v, float sc, float sh, bool has_res, float rv, bool relu) {
  float y = __fadd_rn(__fmul_rn(v, sc), sh);
  if (has_res) y = __fadd_rn(y, rv);
  if (relu) y = (y < 0.f) ? 0.f : y;
  return y;
}
// ... on the four pixels of one channel a lane stores as a float4 at out + idx
__device__ inline float4 epi_val4(const Epi& ep, float sc, float sh, size_t idx, float a0, float a1, float a2, float a3) {
  const bool hr = ep.res != nullptr, rl = ep.relu != 0;
  float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (hr) rv = *reinterpret_cast<const float4*>(ep.res + idx);
  return make_float4(epi_val(a0, sc, sh, hr, rv.x, rl), epi_val(a1, sc, sh, hr, rv.y, rl),
                     epi_val(a2, sc, sh, hr, rv.z, rl), epi_val(a3, sc, sh, hr, rv.w, rl));
}

// The residual as a view (Epi::rvw0 / rvw1, the code instances alone): the element that adds to out (b, o, pixel p
// of a wo-wide map), +0.0f outside the view's channels -- the add itself stays a real one, so that a -0.0 becomes
// +0.0 as torch's add of the padded zero makes it.
__device__ inline float epi_view(const Epi& ep, int b, int o, int p, int wo) {
  const ResView v = res_view(ep.rvw0, ep.rvw1);
  const int c = o - v.c0;
  if ((unsigned)c >= (unsigned)v.cr) return 0.f;
  const int h = p / wo, w = p - h * wo;
  return ep.res[(((size_t)b * v.cr + c) * v.h + (size_t)v.s * h) * v.w + v.s * w];
}
// ... epi_val4 of a code instance: the four pixels p .. p + 3 of one output row (wo % 4 == 0, checked on the host)
// of image b, channel o; a view is read with four scalar loads, a full residual is epi_val4's float4
__device__ inline float4 epi_val4v(const Epi& ep, float sc, float sh, size_t idx, int b, int o, int p, int wo, float a0,
                                   float a1, float a2, float a3) {
  if (ep.rvw1 == 0) return epi_val4(ep, sc, sh, idx, a0, a1, a2, a3);  // (block-uniform)
  // (the two words through opaque copies: unpacked here, at the store, and not into five scalar registers held
  // across the whole m-tile loop)
  uint32_t w0 = ep.rvw0, w1 = ep.rvw1;
  asm volatile("" : "+s"(w0), "+s"(w1));
  const ResView v = res_view(w0, w1);
  const bool rl = ep.relu != 0;
  float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
  const int c = o - v.c0;
  if ((unsigned)c < (unsigned)v.cr) {
    const int h = p / wo, w = p - h * wo;
    const float* src = ep.res + (((size_t)b * v.cr + c) * v.h + (size_t)v.s * h) * v.w + v.s * w;
    rv = make_float4(src[0], src[v.s], src[2 * v.s], src[3 * v.s]);
  }
  return make_float4(epi_val(a0, sc, sh, true, rv.x, rl), epi_val(a1, sc, sh, true, rv.y, rl),
                     epi_val(a2, sc, sh, true, rv.z, rl), epi_val(a3, sc, sh, true, rv.w, rl));
}

// tensor.type(torch.int8): truncate toward zero, keep the low byte (wraps).  NaN -> 0.
__device__ inline int to_i8_wrap(float v) {
  if (!(fabsf(v) < 2147483520.f)) return 0;
  int t = (int)v;
  return (int)(int8_t)(t & 0xFF);
}

__device__ inline int clamp_i8(float v) {
  v = rintf(v);
  v = fminf(fmaxf(v, -127.f), 127.f);
  return (int)v;
}

// torch.clamp: NaN propagates.
__device__ inline float clamp_nan(float v, float lo, float hi) {
  return (v != v) ? v : fminf(fmaxf(v, lo), hi);
}

// The fp16 store of the partial sums (lsq.py:169,177): an integer ps rounded to half.
// grad_scale(x, s) forward value: (x - x*s).detach() + x*s  (_quan_base.py grad_scale)
__device__ inline float grad_scale_value(float x, float s) {
  const float yg = x * s;
  const float d = x - yg;
  return d + yg;
}

// The activation code of a value entering a layer with step size sa and clamp maximum qp (an integer, <= 254):
// the quantiser's own chain (act_words_tab) -- one IEEE division, the clamp, rint -- and qp + 1 for a NaN.
__device__ inline uint32_t act_code(float y, float sa, float qp) {
  const float r = rintf(clamp_nan(y / sa, 0.f, qp));
  return (r == r) ? (uint32_t)(int)r : (uint32_t)(int)qp + 1u;
}
// the codes of the float4 a lane stores, one byte per pixel, lowest byte first: one 32-bit store at oq + idx
__device__ inline uint32_t act_code4(const float4& y, float sa, float qp) {
  return act_code(y.x, sa, qp) | (act_code(y.y, sa, qp) << 8) | (act_code(y.z, sa, qp) << 16) |
         (act_code(y.w, sa, qp) << 24);
}
// The store of a code instance (cimq_module_forward_codes): the float4 y at out + idx unless
// CIMQ_CODES_NO_FLOAT, and with ep.oq the codes of y for the consumer layer, one 32-bit store at oq + idx.
// The consumer's step size is the module prologue's own expression on its parameter (grad_scale_value).
__device__ inline void store_codes4(const Epi& ep, float* __restrict__ out, size_t idx, const float4& y) {
  if (!ep.nofloat) *reinterpret_cast<float4*>(out + idx) = y;
  if (ep.oq) {
    const float osa = grad_scale_value(ep.oalpha[0], ep.ogs);
    *reinterpret_cast<uint32_t*>(ep.oq + idx) = act_code4(y, osa, ep.oqp);
  }
}

// round_pass(v) forward value: (v.round() - v).detach() + v  (lsq.py:29-32)
__device__ inline float round_pass_value(float v) {
  const float r = rintf(v);
  return (r - v) + v;
}

__device__ inline float ps_half(int p) { return __half2float(__float2half_rn((float)p)); }

// u = ps * sw * sa in fp32, in the reference's order (lsq.py:195).
__device__ inline float u_of(int p, float sw, float sa) {
  float ps = ps_half(p);
  float t = ps * sw;
  return t * sa;
}

// The ADC of lsq.py:197-230 evaluated literally for one partial sum (no threshold shortcut).
__device__ inline float adc_literal(int p, int mode, float sw, float sa, float alpha, float qn,
                                    float qp) {
  float u = u_of(p, sw, sa);
  if (mode == ADC_FP) return u;
  if (mode == ADC_SIGN) {
    float s = (u > 0.f) ? 1.f : ((u < 0.f) ? -1.f : ((u != u) ? u : 0.f));
    return s * alpha;
  }
  if (mode == ADC_TERNARY) {
    float v = u / alpha;
    float q = clamp_nan(rintf(v), qn, qp);
    return q * alpha;
  }
  float d = sw * sa;
  float v = u / d;
  float q = clamp_nan(rintf(v), qn, qp);
  float t = q * sw;
  return t * sa;
}

// The backward's rescaled partial sum (lsq.py:257-267).
__device__ inline float psb_literal(int p, int mode, float sw, float sa, float alpha) {
  if (mode == ADC_SIGN || mode == ADC_TERNARY) return u_of(p, sw, sa) / alpha;
  return ps_half(p);
}

// STE mask (lsq.py:310-313): gradient passes unless clamped.
__device__ inline bool ste_pass(float psb, float thr_hi, float thr_lo) {
  return !(psb >= thr_hi || psb <= thr_lo);
}

// ADC code used by grad_alpha (lsq.py:321-332), literal form.
__device__ inline float alpha_code_literal(float psb, int mode, float qn, float qp, float thr_hi,
                                           float thr_lo) {
  if (mode == ADC_SIGN) return (psb > 0.f) ? 1.f : ((psb < 0.f) ? -1.f : ((psb != psb) ? psb : 0.f));
  float q = rintf(psb);
  if (psb >= thr_hi) q = qp;
  if (psb <= thr_lo) q = qn;
  return q;
}

// ---------------------------------------------------------------------------------------
// ADC variants (cimq_conv_desc.adc_variant), evaluated literally per partial sum
// ---------------------------------------------------------------------------------------
__device__ inline bool has_alpha(const Geo& g) {
  return g.mode == ADC_SIGN || g.mode == ADC_TERNARY || g.variant == VAR_SHIFT_ROUND || g.variant == VAR_SHIFT_SIGN;
}
__device__ inline bool is_shift(const Geo& g) { return g.variant == VAR_SHIFT_ROUND || g.variant == VAR_SHIFT_SIGN; }
// torch.sign: NaN propagates
__device__ inline float sign_nan(float v) { return (v > 0.f) ? 1.f : ((v < 0.f) ? -1.f : ((v != v) ? v : 0.f)); }

// the partial sum as the ADC input sees it, times sw * sa (lsq.py:195): the fp16 store of the
// library (lsq.py:169) or the int8 buffer of the scale/shift ver2 Function (scale_shift.py:401)
__device__ inline float u_var(const Geo& g, int p, float sw, float sa) {
  float ps = ps_half(p);
  if (g.ps_int8) ps = (float)(int8_t)(((int)ps) & 0xFF);
  const float t = ps * sw;
  return t * sa;
}

// Philox4x32-10 (Salmon et al., SC'11): counter-based, so a draw depends only on (key, counter)
__device__ inline void philox4x32(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1;
    c[3] = (uint32_t)p0;
    c[0] = n0;
    c[2] = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// number of draws U ~ [0,1) (24-bit) with ceil(s - U) == 1, i.e. U < s, out of 50 (lsq.py:214-217);
// draws d = 0..49 of stream `which` of element `eid`
__device__ inline float bernoulli50(float s, uint64_t eid, uint32_t which, uint32_t k0, uint32_t k1) {
  if (s <= 0.f) return 0.f;   // ceil(0 - U) = 0 for every U in [0, 1)
  if (s >= 1.f) return 50.f;  // ceil(1 - U) = 1
  float n = 0.f;
  for (uint32_t blk = 0; blk < 13; ++blk) {
    uint32_t c[4] = {(uint32_t)eid, (uint32_t)(eid >> 32), which, blk};
    philox4x32(c, k0, k1);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (blk * 4 + e < 50) {
        const float u = (float)(c[e] >> 8) * 5.9604644775390625e-8f;  // 2^-24
        n += (s - u > 0.f) ? 1.f : 0.f;                                // ceil(s - u) with s - u in (-1, 1)
      }
    }
  }
  return n;
}

// stochastic 1.5-bit ADC of lsq.py:205-221 for one partial sum (u = ps*sw*sa)
__device__ inline float adc_stochastic(const Geo& g, float u, float alpha, uint64_t eid) {
  const float h = 0.5f * alpha;
  const float z1 = (u - h) / 0.01f, z2 = (u + h) / 0.01f;
  const float s1 = 1.f / (1.f + expf(-z1)), s2 = 1.f / (1.f + expf(-z2));  // torch.sigmoid
  const float n1 = bernoulli50(s1, eid, 0u, g.seed_lo, g.seed_hi);
  const float n2 = bernoulli50(s2, eid, 1u, g.seed_lo, g.seed_hi);
  const float a = n1 / 50.f, b = n2 / 50.f;
  const float v = (a + b) - 1.f;
  return clamp_nan(rintf(v), g.qn, g.qp) * alpha;
}

// ADC output (before the shift-and-add mask) of one partial sum, every variant
__device__ inline float adc_value(const Geo& g, int p, float sw, float sa, float alpha, float beta, uint64_t eid) {
  if (g.variant == VAR_SHIFT_ROUND) {
    const float v = (u_var(g, p, sw, sa) - beta) / alpha;  // scale_shift.py:421
    const float t = clamp_nan(rintf(v), g.qn, g.qp) * alpha;  // :424-425
    return t + beta;
  }
  if (g.variant == VAR_SHIFT_SIGN) {
    const float v = (u_var(g, p, sw, sa) - beta) / alpha;  // scale_shift.py:202
    const float t = sign_nan(v) * alpha;                    // :209-211
    return t + beta;
  }
  if (g.variant == VAR_STOCHASTIC) return adc_stochastic(g, u_of(p, sw, sa), alpha, eid);
  return adc_literal(p, g.mode, sw, sa, alpha, g.qn, g.qp);
}

// the backward's rescaled partial sum (lsq.py:257-267; scale_shift.py:469 / :202)
__device__ inline float psb_value(const Geo& g, int p, float sw, float sa, float alpha, float beta) {
  if (is_shift(g)) return (u_var(g, p, sw, sa) - beta) / alpha;
  return psb_literal(p, g.mode, sw, sa, alpha);
}

// per-partial-sum factor of grad_alpha (times g, summed over the batch and pixels)
__device__ inline float alpha_term(const Geo& g, float b) {
  if (g.variant == VAR_SHIFT_ROUND) {  // scale_shift.py:488-495: round(ps) - ps, Qp / Qn where clamped
    if (b >= g.thr_hi) return g.qp;
    if (b <= g.thr_lo) return g.qn;
    return rintf(b) - b;
  }
  if (g.variant == VAR_SHIFT_SIGN) return sign_nan(b);  // scale_shift.py:281
  return alpha_code_literal(b, g.mode, g.qn, g.qp, g.thr_hi, g.thr_lo);
}

// per-partial-sum factor of grad_beta: the clamped region (ver2, :496-501) or 1 (adcless, :287)
__device__ inline float beta_term(const Geo& g, float b) {
  if (g.variant == VAR_SHIFT_SIGN) return 1.f;
  return (b >= g.thr_hi || b <= g.thr_lo) ? 1.f : 0.f;
}

// fp32 -> bf16 round-to-nearest-even (finite inputs) and back
__device__ inline uint16_t bf16_bits(float f) {
  uint32_t u = __float_as_uint(f);
  uint32_t r = u + 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(r >> 16);
}
__device__ inline float bf16_to_f(uint16_t h) { return __uint_as_float(((uint32_t)h) << 16); }

// Split a float into hi + mid + lo bf16 parts (24 significant bits): the three-term
// decomposition that gives fp32-accurate products on the bf16 MFMA when the other operand
// is a small integer (exact in bf16).
__device__ inline void split3(float a, uint16_t& hi, uint16_t& mid, uint16_t& lo) {
  hi = bf16_bits(a);
  float r1 = a - bf16_to_f(hi);
  mid = bf16_bits(r1);
  float r2 = r1 - bf16_to_f(mid);
  lo = bf16_bits(r2);
}

__device__ inline v8bf as_v8bf(v4i x) { return __builtin_bit_cast(v8bf, x); }
__device__ inline v4i as_v4i(v8bf x) { return __builtin_bit_cast(v4i, x); }

// (v_l + v_{l^16}) + (v_{l^32} + v_{l^48}) in every lane: the sum over the four 16-lane rows of a wave,
// in __shfl_xor(16)-then-(32)'s order and rounding (each add is commutative, so bit-identical to it), on
// the gfx950 row-swap permutes (VALU) instead of two LDS-crossbar ds_bpermute round trips
__device__ inline float rows4_sum(float v) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  const float h = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  const auto c = __builtin_amdgcn_permlane32_swap(__float_as_uint(h), __float_as_uint(h), false, false);
  return __uint_as_float(c[0]) + __uint_as_float(c[1]);
}

// fp32 -> three bf16 parts (hi + mid + lo), 8 values -> 3 MFMA operands (split3x8)
// (a, b) -> bf16 hi / mid / lo pairs, low half a: round-to-nearest-even conversions and exact fp32
// remainders (hi + mid + lo reproduces a to fp32 accuracy), one v_cvt_pk_bf16_f32 per level for both values
__device__ inline uint32_t pk_bf16(float a, float b) {
  uint32_t r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ inline void split3_pk(float a, float b, uint32_t& hi, uint32_t& mid, uint32_t& lo) {
  hi = pk_bf16(a, b);
  float ra = a - __uint_as_float(hi << 16), rb = b - __uint_as_float(hi & 0xffff0000u);
  mid = pk_bf16(ra, rb);
  ra = ra - __uint_as_float(mid << 16);
  rb = rb - __uint_as_float(mid & 0xffff0000u);
  lo = pk_bf16(ra, rb);
}
__device__ inline void split3x8(const float (&v)[8], v8bf& bh, v8bf& bm, v8bf& bl) {
  v4i h, m, l;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    uint32_t a, b, c;
    split3_pk(v[2 * e], v[2 * e + 1], a, b, c);
    h[e] = (int)a;
    m[e] = (int)b;
    l[e] = (int)c;
  }
  bh = __builtin_bit_cast(v8bf, h);
  bm = __builtin_bit_cast(v8bf, m);
  bl = __builtin_bit_cast(v8bf, l);
}

// literal (threshold-free) per-partial-sum paths, kept out of line: degenerate alpha / scales
__device__ __noinline__ inline float adc_literal_sum(v4i ps, int mode, float sw, float sa, float al, float qn,
                                                    float qp, float mk, int r) {
  return adc_literal(ps[r], mode, sw, sa, al, qn, qp) * mk;
}
__device__ __noinline__ inline float ste_literal(int p, int mode, float sw, float sa, float al, float thr_hi,
                                                float thr_lo) {
  const float bb = psb_literal(p, mode, sw, sa, al);
  return ste_pass(bb, thr_hi, thr_lo) ? 1.f : 0.f;
}
__device__ __noinline__ inline float code_literal(int p, int mode, float sw, float sa, float al, float qn, float qp,
                                                 float thr_hi, float thr_lo) {
  const float bb = psb_literal(p, mode, sw, sa, al);
  return alpha_code_literal(bb, mode, qn, qp, thr_hi, thr_lo);
}
// the shift ADC's literal path (shift_fast layers with a degenerate alpha / beta / scale): adc * mask
// (scale_shift.py:421-429) and the state bits of the partial sum (v = (u - beta) / alpha: STE pass
// unless v >= Qp + 1e-5 or v <= Qn - 1e-5, :469-484; code clamp(rint(v), -1, 1))
// (scalar arguments only, as the helpers above: a Geo by reference would put it on the stack and
// cost the whole kernel registers; shift_fast fixes ps_int8 = 0 and the range -1 .. 1)
__device__ __noinline__ inline float shift_adc_literal(int p, float sw, float sa, float al, float be, float mk) {
  const float u = (ps_half(p) * sw) * sa;  // u_var without the int8 buffer
  const float v = (u - be) / al;
  const float t = clamp_nan(rintf(v), -1.f, 1.f) * al;
  return (t + be) * mk;
}
__device__ __noinline__ inline uint32_t shift_state_literal(int p, float sw, float sa, float al, float be,
                                                           float thr_hi, float thr_lo) {
  const float v = (((ps_half(p) * sw) * sa) - be) / al;
  const bool pass = !(v >= thr_hi || v <= thr_lo);
  const float code = clamp_nan(rintf(v), -1.f, 1.f);
  return (pass ? 1u : 0u) | ((code != 0.f) ? 2u : 0u) | ((code < 0.f) ? 4u : 0u);
}

// state bits of one partial sum: bit 0 STE pass (lsq.py:310-313), bit 1 ADC code != 0, bit 2
// ADC code < 0 (lsq.py:321-332)
__device__ inline uint32_t st_bits(bool pass, float code) {
  return (pass ? 1u : 0u) | ((code != 0.f) ? 2u : 0u) | ((code < 0.f) ? 4u : 0u);
}

// shift a bit in: x * 2 + c in one v_addc_co_u32 whose carry-in is the compare's lane mask
// (the compiler spends a cndmask + shift/or on the plain expression)
__device__ inline uint32_t shin(uint32_t x, uint64_t m) {
  uint32_t r;
  uint64_t co;
  asm("v_addc_co_u32_e64 %0, %1, %2, %2, %3" : "=v"(r), "=s"(co) : "v"(x), "s"(m));
  return r;
}
// ternary ADC term: hi ? cf : (lo ? -cf : 0) from the two compare masks (two cndmasks; the
// plain expression makes the compiler rematerialise the masks as 0/1 vectors)
__device__ inline float adc3(float cf, uint64_t mhi, uint64_t mlo) {
  float a, r;
  asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(a) : "v"(cf), "s"(mhi));
  asm("v_cndmask_b32_e64 %0, %1, -%2, %3" : "=v"(r) : "v"(a), "v"(cf), "s"(mlo));
  return r;
}

}  // namespace cimq
