// cimq_types.h -- the plain types and constants the host plans (cimq_host.h) and the kernels share: problem
// geometry, parameter tables, the plan structs the host fills and passes by value, the LDS layouts and table
// sizes a plan reads.  No device code.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cimq {

#define WAVE 64  // lanes per wavefront (cimq_device.h refuses anything else)

typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));

enum AdcMode { ADC_FP = 0, ADC_SIGN = 1, ADC_TERNARY = 2, ADC_MULTI = 3 };
// cimq_conv_desc.adc_variant & 0xFF (include/cimq.h CIMQ_ADC_*)
enum AdcVariant { VAR_LIBRARY = 0, VAR_STOCHASTIC = 1, VAR_SHIFT_ROUND = 2, VAR_SHIFT_SIGN = 3 };

// Problem geometry, computed once on the host (cimq_api.hip) and passed by value.
struct Geo {
  int B, C, H, W, O, KH, KW, SH, SW, PH, PW, Ho, Wo;
  int P, M, K, KHW, HW;
  int xbar, T, KS, KTP;    // KS: 64-deep int8 K-steps per tile, KTP: LDS row pitch (bytes)
  int FBT;                 // 16-wide f-blocks per tile (ceil(xbar/16))
  int nbw, nba, bsw, bsa, NBP;  // NBP: bytes per input element in the packed act-code array
  int Opad, OB16, NBLK, NKS;    // Opad=roundup(O,16); NBLK = nbw*Opad/16; NKS = ceil(NBLK/2)
  int mode;
  float qn, qp, thr_hi, thr_lo;  // ADC range; backward clamp thresholds fl32(Qp+1e-5), fl32(Qn-1e-5)
  int input_kind;
  float lsq_qp;
  int psmax;               // bound on |partial sum| used by the threshold search
  long long Nin;           // B*C*H*W
  int onchw;               // out / grad_out layout: 0 = [B, P, O] (the Function's), 1 = NCHW (the module's)
  int variant;             // AdcVariant; anything but VAR_LIBRARY runs the literal (general) kernels
  int ps_int8;             // partial sums pass an int8 buffer before the ADC (scale_shift.py:401)
  // host side, cimq_conv_desc.options (two halves of what was one int, so that the struct every kernel takes by
  // value keeps its size and its offsets): CIMQ_OPT_RECOMPUTE -- the module backward recomputes partial sums --
  // and CIMQ_OPT_INFERENCE -- forward only, nothing written that a backward would read
  short recompute, inference;
  uint32_t seed_lo, seed_hi;  // VAR_STOCHASTIC: Philox key
  const unsigned char* wbase;  // host side: the weight-side ctx regions (cimq_lsq_desc.wprep); null: inside ctx
};
static_assert(sizeof(Geo) == 200, "Geo is every kernel's first argument: keep its size and offsets");

// Per-(tile i, a-slice j, w-slice k, out-channel o) ADC / STE parameters, SoA.
// index: ((i*nba + j)*nbw + k)*Opad + o
struct Params {
  int* thi;     // forward: ps >= thi -> code +1   (ternary mode)
  int* tlo;     // forward: ps <= tlo -> code -1
  int* mlo;     // backward: STE passes iff (unsigned)(ps - mlo) <= (unsigned)mhi (lsq.py:310-313)
  int* mhi;     //   ... mhi holds the interval span
  float* coef;  // alpha_q * binary_mask  (ternary / sign)
  float* alpha; // alpha_q (literal paths)
  float* ckj;   // [3][nbw*nba]: mask as float, cE = 2^-(bsa*j)*mask, cD = 2^-(bsw*k)*mask
  int* flags;   // [0]: literal ADC (degenerate alpha / scales), [1..3] reserved
  float* beta;  // shift of the scale + shift ADC variants (0 otherwise)
  float* bsum;  // [Opad]: sum over (i, k, j) of beta * binary_mask (shift_fast forward)
};

// The output epilogue of cimq_module_forward_epilogue (cimq_epilogue, include/cimq.h), the last argument of the
// forward kernels: only their epilogue instances (forward only, CIMQ_OPT_INFERENCE) read it.
struct Epi {
  const float* scale;  // [O]
  const float* shift;  // [O]
  const float* res;    // null, or the residual in out's layout (NCHW)
  int relu;            // CIMQ_EPI_RELU
  // activation codes (cimq_act_codes, cimq_module_forward_codes): read by the code instances alone -- the fields
  // follow the epilogue's, so every other instance finds its arguments where they were
  int nofloat;           // CIMQ_CODES_NO_FLOAT: out is not written
  const uint8_t* xq;     // null, or the input as codes ([B, C, H, W] bytes) in place of the fp32 x
  uint8_t* oq;           // null, or where the output's codes go ([B, O, Ho, Wo] bytes)
  const float* oalpha;   // [1]: the consumer's alpha_act
  float ogs;             // the consumer's gradient-scale factor
  float oqp;             // the consumer's clamp maximum, an integer in [1, 254]
  // the residual as a view (cimq_net_layer's res_c0 / res_stride, the option-A shortcut): read by the code
  // instances alone, trailing for the same reason.  rvw1 0: res has out's layout.  Otherwise res is
  // [B, rcr, rh, rw] and out (b, o, h, w) adds res[b, o - rc0, rs * h, rs * w] where rc0 <= o < rc0 + rcr, +0.0f
  // elsewhere.  Two packed words (two scalar registers, unpacked at the store): rvw0 = rc0 | rcr << 16,
  // rvw1 = rh | rw << 15 | (rs - 1) << 30 (rh >= 1, so a view's rvw1 is never 0)
  uint32_t rvw0, rvw1;
};
constexpr int kViewMaxDim = 32767;  // rh, rw (15 bits each); rc0, rcr fit 16 bits likewise
struct ResView { int c0, cr, s, h, w; };
__host__ __device__ inline ResView res_view(uint32_t w0, uint32_t w1) {
  return ResView{(int)(w0 & 0xffffu), (int)(w0 >> 16), (int)(w1 >> 30) + 1, (int)(w1 & 0x7fffu), (int)((w1 >> 15) & 0x7fffu)};
}
inline void set_res_view(Epi* ep, int c0, int cr, int s, int h, int w) {
  ep->rvw0 = (uint32_t)c0 | (uint32_t)cr << 16;
  ep->rvw1 = (uint32_t)h | (uint32_t)w << 15 | (uint32_t)(s - 1) << 30;
}

// What a forward kernel instance does with its output: a template argument of cim_fwd_v3_kernel, cim_fwd5_kernel and
// dense_fwd*_kernel.  Each mode includes the one before it; fwd_mode_of (cimq_host.h) names a call's mode.
enum class FwdMode : int {
  TRAIN,  // out, and what the backward reads: the state words, the backward ctx words
  INFER,  // forward only (CIMQ_OPT_INFERENCE): out alone -- no state words, none of their bits, no backward words
  EPI,    // ... with the output epilogue (Epi) on the values about to be stored; no earlier mode reads the Epi
  CODES,  // ... with activation codes in (Epi::xq), out (Epi::oq) or both: block-uniform branches on the Epi
  VIEW,   // ... with the residual read as a view (Epi::rvw0 / rvw1, cimq_net_forward's option-A shortcut)
};
constexpr bool has_epi(FwdMode m) { return m >= FwdMode::EPI; }
constexpr bool has_codes(FwdMode m) { return m >= FwdMode::CODES; }
constexpr bool has_view(FwdMode m) { return m >= FwdMode::VIEW; }
constexpr bool writes_state(FwdMode m) { return m == FwdMode::TRAIN; }
// What cim_fwd_v3_kernel does with the state words of a compact format (CST 2 / 3 / 8): it writes them (also the
// one form of CST 0, which writes none in any call); none, because cim_bwd_c1_kernel recomputes them (a training
// instance that a forward-only call runs as it is); forward only: no state bits on either ADC path, no words via xcb
enum class FwdState : int { WRITE, RECOMPUTE, NONE };

__host__ __device__ inline int pidx(const Geo& g, int i, int j, int k, int o) {
  return ((i * g.nba + j) * g.nbw + k) * g.Opad + o;
}

// The scale / shift "round" ADC of Conv2dLSQCiM(adc_shift=True) on the threshold fast path: 1.5 bits
// with the library's range (codes -1, 0, 1), the library's fp16 partial sums (no int8 buffer), every
// |ps| exact in fp16.  v = (u - beta) / alpha is then a monotone step function of the integer ps,
// captured by integer thresholds like the library ADC; the output gains sum beta * mask per channel.
__host__ __device__ inline bool shift_fast(const Geo& g) {
  return g.variant == VAR_SHIFT_ROUND && g.mode == ADC_TERNARY && !g.ps_int8 && g.qp == 1.f && g.qn == -1.f &&
         g.psmax <= 2048;
}

// host-computed plan of the fast path (cimq_kernels_v3.hip; cimq_host.h: v3_plan)
struct V3 {
  int lw;          // log2(Wo)
  int RH;          // strip patch rows: (64/Wo - 1)*SH + KH
  int obm;         // forward: 16-channel output blocks per block (1, 2 or 4)
  int WP;          // patch row length: W + 2*PW
  int RI, nbands;  // grad_x: owned input rows per block, bands per image
  int RHB;         // grad_x: max band patch rows
  int NPB;         // grad_x: max output pixels per band, rounded up to 16
  int fwd_res;     // forward: every tile's weights / thresholds resident in LDS
  int nmt;         // M / 64
  int NCG;         // grad_w: max input channels one tile touches
  int NCBT;        // grad_x: max 16-channel blocks one tile touches
  int CB;          // grad_x: 16-channel blocks of the output tile grid (ceil(C/16))
  int NT;          // grad_x: max output tiles (16 positions x 16 channels) per band
  int pf;          // forward, non-resident tiles: the next tile's weight side prefetched in registers
};

// ... of the v7 backward (cimq_v7.hip; v7_plan)
struct V7 {
  int lw;       // log2(Wo)
  // grad_x (v8: ring fold)
  int NCPBT;    // (c, kh)-row blocks of 4 per tile (wcy operand)
  int SWD;      // segment width: min(16, Wo) output columns per 16-lane MFMA column group
  int NSEG;     // segments per output row
  int NRS;      // output rows per step (64 pixels)
  int RSLOT;    // ring rows (NRS + 2)
  int NPART;    // waves sharing one pixel group (split over (c, kh)-blocks)
  int lwin, lcin;  // log2(W), log2(C) (the v7 path takes power-of-two W and C)
  // grad_x
  int RB;       // input rows owned by one block
  int nbands;   // bands per image
  int FBX;      // f-blocks per tile (FBT)
  // grad_w
  int NSLOT;    // staged input rows per 128-pixel stage
  int CPITCH;   // plane channel pitch (bf16 elements)
  int nstage;   // 128-pixel stages per chunk
  int nchunks;  // pixel chunks
  int whole;    // 1: a stage is 128/P whole images; 0: a stage is 128/Wo rows of one image
  int CPL;      // channels per staged plane: min(16, C)
  int NTL;      // most crossbar tiles touching one 16-channel block (grad_alpha LDS regions)
  int GSH;      // grad_x, NPART > 1, at most 2 o-blocks: the NPART waves of a pixel group build disjoint G chunks and
                // exchange them through LDS (else every wave builds all of them)
  int KWP;      // grad_w: (slice j, kw) plane pitch (bf16 elements, >= CPL * CPITCH; gw_pitches)
};

// ... of the fused backward (cimq_fused.hip; v9_plan)
struct V9 {
  int lw;        // log2(W)
  int R;         // output rows per step (64 / W)
  int nsteps;    // H / R
  int SWD, NSEG; // ring segments (as V7): min(16, W) columns, W / SWD per row
  int RSLOT;     // ring rows
  int NCPBT;     // (c, kh)-row blocks of 4 per tile (the v8 grad_x operand wcy)
  int lcin;      // log2(C), or -1
  int NCG;       // most input channels one tile touches (staged plane channels)
  int CPITCH;    // plane channel pitch (bf16): PROWS * W + 8 (the 8-element zero pad)
  int KWP;       // (j, kw) plane pitch (bf16)
  int PROWS;     // staged input rows per step: R + 2
  int NGRP;      // 16-row groups of K
  int gwl;       // 1: grad_w accumulates in LDS across steps; 0: one step per image, units write the slab
  int nitems;    // plane staging items per unit: NCG * PROWS * W / 8 (<= 512)
  unsigned o_ring, o_cel, o_red, o_plane, o_gwl, o_gal, o_st, o_g, lds;  // LDS layout (bytes)
};

// ... of the first conv's backward (cimq_c1.hip; c1_plan)
struct VC1 {
  int lw;       // log2(W)
  int R;        // output rows per step (128 / W)
  int nsteps;   // H / R
  int RH, WP;   // staged input rows per step ((R - 1) + 3) and their word pitch (W + 2)
  int SWD, NSEG, RSLOT;  // ring geometry (as V7)
  int NCPBT;    // wcy blocks
  int lcin;     // log2(C) or -1
  unsigned o_xp, o_hp, o_ptab, o_prm, o_cel, o_g, o_ring, o_gal, o_red, o_e, o_wk, o_wc, lds;
};

constexpr int kF5MaxTc = 8;   // (tile, channel-block) pairs: 2 / 4 / 8 for C = 16 / 32 / 64 at xbar 128
constexpr int kF5MaxGrp = 4;  // tile groups

// ... of the w3a3 module forward (cimq_fwd5.hip; f5_plan)
struct F5 {
  int lwo;                 // log2(Wo)
  int lwi;                 // log2(W)
  int codes;               // 1: the ctx holds one code byte per element (Route::codes: grad_w is cim_bwd_gw5_kernel)
  int IPM;                 // images per 128-pixel m-tile (1: the m-tile is R output rows of one image)
  int R, RH, WP;           // output rows per image slot, patch rows (R-1)*SH + 3, patch row length W + 2
  int NCBP;                // channel blocks one patch holds (the widest group's span)
  int nmt;                 // M / 128
  int ntc;                 // (tile, channel-block) pairs
  int ngrp;                // tile groups
  int tcmax;               // most pairs in one group
  // (int tables: the kernel indexes them with wave-uniform runtime indices, which scalar loads serve
  // only at dword granularity -- byte tables became per-lane global loads of the kernel arguments)
  int tc0[kF5MaxTc + 1];  // first pair of tile i (tc0[T] = ntc)
  int tcb[kF5MaxTc];      // channel block of pair t
  int gt0[kF5MaxGrp + 1]; // first tile of group q (gt0[ngrp] = T)
  int gcb0[kF5MaxGrp], gcb1[kF5MaxGrp];  // channel-block span of group q
  int gown[kF5MaxGrp];    // first channel block whose ctx words group q writes
};

// the part of the plan the weight prologue needs (kept small: it travels in every PrepJob)
struct F5W {
  int ntc;
  unsigned char tc0[kF5MaxTc + 1];
  unsigned char tcb[kF5MaxTc];
};
inline F5W f5w_of(const F5& v) {
  F5W w;
  w.ntc = v.ntc;
  for (int i = 0; i <= kF5MaxTc; ++i) w.tc0[i] = v.tc0[i];
  for (int i = 0; i < kF5MaxTc; ++i) w.tcb[i] = v.tcb[i];
  return w;
}

// the code -> ctx word table's entry for out-of-image elements (a zero word; codes are <= 256)
constexpr int kZeroCode = 259;

// ... of the w3a3 grad_w / grad_alpha kernel (cimq_gw5.hip; g5_plan)
struct G5 {
  int lwo;     // log2(Wo)
  int lwi;     // log2(W)
  int codes;   // 1: the ctx holds one activation code byte per element (the forward was cim_fwd5_kernel with
               // Route::codes): expanded through the act word table, as the forward's staging does
  int IPM;     // images per 128-pixel m-tile (1: the m-tile is R output rows of one image)
  int R, RH, WP;  // output rows per image slot, staged input rows R + 2, patch row length W + 2
  int nmt;     // M / 128
  int nst;     // m-tiles per block (chunk)
  int nchunks; // blocks = slab chunks
};

// ... of the per-input-pixel grad_x kernel (cimq_gx5.hip; x5_plan)
struct X5 {
  int nmt;     // H / 4 * B: m-tiles of four input rows
  int tpi;     // m-tiles per image
  int CBN;     // 16-channel input blocks (1 or 2) = 16-channel output halves
  int NPG;     // 16-pixel groups per m-tile: W / 4 (8 or 4); waves = NPG * CBN = 8
  int lw;      // log2(W)
};

// ... of the recompute backward (cimq_r6.hip; r6_plan)
struct R6 {
  int tc0[3];  // first (tile, channel-block) pair of tile i in cim_fwd5_kernel's operand (f5_plan)
  int ntc;     // pairs
  int nmt;     // m-tiles per image (H / 4)
};

// geometry of the 16-channel layer (r6_plan checks it)
constexpr int kR6C = 16, kR6W = 32, kR6R = 4, kR6T = 2;
constexpr int kR6KO = 3 * kR6C;          // kappa (k, o) per tile: 48
constexpr int kR6NK = kR6T * kR6KO;      // kappa per G-patch pixel: 96 = 3 K-steps
constexpr int kR6KSG = kR6NK / 32;
constexpr int kR6WxItems = 9 * kR6KSG * 64;  // 16-byte items of its gx operand (wx6_item)

// LDS layout of cim_bwd_r6_kernel (bytes; 159.3 KB: one workgroup per CU)
struct R6L {
  static constexpr int RP = kR6R + 2, WP = kR6W + 2;
  static constexpr int GPX = kR6NK * 2 + 16;  // G-patch pixel pitch: 13 16-B slots, a wave's 16 pixels on distinct slots
  static constexpr int GROW = WP * GPX;       // one G-patch row of one plane
  static constexpr int GPL = kR6R * GROW;     // one plane
  static constexpr int EXP = 36;              // exchange pitch (floats per input channel): 16-B writes on distinct banks
  static constexpr int O_XP = 0;                             // forward slice patch [RP][WP][3 slices][16 ch] int8 (f5_off)
  static constexpr int O_XH = O_XP + RP * WP * 48;           // ctx slices, A-ready [C][RP][WP] x (bf16 x0|x1, x2|0)
  static constexpr int O_GP = O_XH + kR6C * RP * WP * 8;     // G patch [3 planes][R][WP][NK] bf16; exchange aliases it
  static constexpr int O_CA = O_GP + 3 * GPL;                // carried partial rows [2][C][W] fp32
  static constexpr int O_WX = O_CA + 2 * kR6C * kR6W * 4;    // gx operand [9][KSG][64] x 16 B
  static constexpr int O_PR = O_WX + kR6WxItems * 16;        // ADC / STE thresholds [T][9 kj][16 o] int4
  static constexpr int O_AL = O_PR + kR6T * 9 * 16 * 16;     // act word table [Qp + 2][fwd, bwd]
  static constexpr int O_CE = O_AL + 260 * 8;                // cE_kj [9], cD_kj [9]
  static constexpr int LDS = O_CE + 32 * 4;
};
static_assert(R6L::LDS <= 160 * 1024, "r6 LDS budget");
static_assert(9 * 8 * 64 * 16 <= 3 * R6L::GPL, "r6 gw reduction buffer");
static_assert(2 * kR6T * 9 * 8 * 16 * 4 <= 3 * R6L::GPL, "r6 grad_alpha reduction buffer");

// The ctx's code -> word table region (CtxLayout::alut, 1,280 bytes) also carries a format word at entry
// kCalFlag: cim_fwd5_kernel writes kCodesMagic there when it stores one activation code byte per ctx element
// (Route::codes), and cim_bwd_gw5_kernel's code-byte instance checks it -- a ctx written in the other format
// (a forward / backward planned differently, e.g. a tuning knob changed in between) yields NaN grad_w and
// grad_alpha partials instead of silently reading words as codes.
constexpr int kCalFlag = 300;
constexpr uint32_t kCodesMagic = 0xC0DE5EEDu;

// the RAW_LSQ activation word table a block builds in LDS (act_lut_build) holds codes below this
constexpr int kActLutMax = 256;

__host__ __device__ inline size_t a16(size_t v) { return (v + 15) & ~(size_t)15; }

// cim_fwd_v3_kernel's dynamic LDS, region by region in order: X(name, bytes) in terms of g (Geo), v (V3), NBP, KS,
// NOB (16-channel output blocks per block), TT (tiles with a resident weight side: T with V3::fwd_res, else 1), nkj.
// The kernel carves its pointers from this list, fwd3_lds_bytes (cimq_host.h: v3_plan) sums it, and the fused
// quantiser's word table follows the last region (launch_fwd_v3).  A list and not a function: the kernel's address
// arithmetic stays in its body token for token.
#define CIMQ_FWD3_LDS(X)                                                                                 \
  X(patch, a16((size_t)g.C * v.RH * v.WP * NBP)) /* [C][RH][WP] words of NBP bytes */                   \
  X(ptab, (size_t)g.T * KS * 64 * 4)              /* [T][KS*64] patch word offsets */                    \
  X(wfl, (size_t)TT * g.nbw * NOB * KS * 1024)    /* [tt][k][ob][ks][64] weight fragments */             \
  X(prm, (size_t)TT * nkj * NOB * 16 * 16)        /* [tt][j][k][NOB*16] int4 thresholds / STE spans */   \
  X(cfl, (size_t)TT * nkj * NOB * 16 * 4)         /* coef, same order */                                 \
  X(ckl, a16((size_t)3 * g.nbw * g.nba * 4))      /* [3][nkj] (Params::ckj) */

// ... of the channel-chunked forward (cimq_wide.hip; wide_plan): the pixel geometry is a V3's (lw, RH, WP, nmt)
struct WideP {
  int tr;   // crossbar tiles per channel chunk (the last chunk may hold fewer)
  int ncx;  // channels the LDS patch holds: the widest chunk's span
  int nch;  // channel chunks: ceil(T / tr)
  int pf;   // compile-time slice counts: the next tile's weight fragments prefetched in registers
};
constexpr int kWideOBM = 4;  // 16-channel output blocks per workgroup (tables sized for four, zero past the last)

// cim_fwd_wide_kernel's dynamic LDS, as CIMQ_FWD3_LDS: in terms of g (Geo), v (V3), wp (WideP), KS, nkj; the fused
// quantiser's word table follows the last region
#define CIMQ_WIDE_LDS(X)                                                                                  \
  X(patch, a16((size_t)wp.ncx * v.RH * v.WP * 4)) /* [ncx][RH][WP] slice words of one channel chunk */    \
  X(ptab, (size_t)wp.tr * KS * 64 * 4)             /* [tr][KS*64] patch word offsets of the chunk's tiles */ \
  X(wfl, (size_t)g.nbw * kWideOBM * KS * 1024)     /* [k][ob][ks][64] weight fragments of one tile */      \
  X(prm, (size_t)nkj * kWideOBM * 16 * 16)         /* [j][k][64] int4 thresholds */                        \
  X(cfl, (size_t)nkj * kWideOBM * 16 * 4)          /* coef, same order */                                  \
  X(ckl, a16((size_t)3 * g.nbw * g.nba * 4))       /* [3][nkj] (Params::ckj) */

}  // namespace cimq
