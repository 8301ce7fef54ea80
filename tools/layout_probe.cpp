// Host-only probe: the module route, the sizes, and the ctx / workspace layouts a source tree's planners give a
// descriptor with the module path's NCHW flag off (the Function entry points) and on (the module entry points).
// It uses only names every revision has (make_geo, ctx_layout, ws_layout, the plan functions, and through the ABI
// cimq_module_route / cimq_query_sizes), so two revisions' outputs can be diffed.  Build against a built tree T:
//   hipcc -O1 -std=c++17 -IT/cim_quantization_amd/csrc tools/layout_probe.cpp -LT/cim_quantization_amd \
//         -l:libcimq.so -Wl,-rpath,T/cim_quantization_amd -o layout_probe
//   layout_probe          bench.RESNET20's distinct w3a3 shapes at B = 256
//   layout_probe --grid   every descriptor of a grid over shapes, bit widths, ADCs, crossbars and options
// (the round-5 first-visit fault)
#include "cimq_host.h"

using namespace cimq;

static void probe(const cimq_conv_desc& d) {
  Geo g;
  if (make_geo(&d, &g) != 0) return;
  printf("B%d C%d O%d H%d s%d k%d w%d adc%g xbar%d var%d in%d opt%d |", d.batch, d.in_channels, d.out_channels, d.in_h,
         d.stride_h, d.kernel_h, d.bits_w, (double)d.adc_bits, d.xbar, d.adc_variant, d.input_kind, d.options);
  int r[3] = {-1, -1, -1};
  const int rc = cimq_module_route(&d, r);
  cimq_sizes z;
  memset(&z, 0, sizeof(z));
  const int rs = cimq_query_sizes(&d, &z);
  printf(" route %d: %d %d %d | sizes %d: %zu %zu %zu %zu %zu |", rc, r[0], r[1], r[2], rs, z.ctx_bytes,
         z.fwd_workspace_bytes, z.bwd_workspace_bytes, z.wprep_bytes, z.module_ctx_bytes);
  for (int n = 0; n < 2; ++n) {
    g.onchw = n;
    const CtxLayout L = ctx_layout(g);
    const WsLayout W = ws_layout(g);
    printf(" ctx%d", n);
    for (size_t v : {L.xcode, L.xhat, L.alut, L.wfrag, L.wf5, L.wg5, L.wx6, L.wgx, L.wcy, L.thi, L.tlo, L.mlo, L.mhi, L.coef,
                     L.alpha, L.beta, L.bsum, L.ckj, L.flags, L.st, L.lsq_scal, L.wbytes, L.total})
      printf(" %zu", v);
    printf(" ws%d", n);
    for (size_t v : {W.gw_slab, W.ga_slab, W.gb_slab, W.ss_slab, W.qtab, W.lsq_part, W.gaq, W.gapart, W.wpart, W.bpo, W.gxu,
                     W.total})
      printf(" %zu", v);
    printf(" %d %d %d |", W.rows, W.nchunks, W.nchunks_bwd);
  }
  const Plan7 p7 = v7_plan(g);
  const Plan9 p9 = v9_plan(g);
  printf(" p7 %d %d %d p9 %d %d %d\n", (int)p7.ok, p7.ok ? p7.v.CPITCH : 0, p7.ok ? p7.v.KWP : 0, (int)p9.ok,
         p9.ok ? p9.v.CPITCH : 0, p9.ok ? p9.v.KWP : 0);
}

static cimq_conv_desc desc(int B, int C, int O, int H, int s, int k, int bits, float adc, int xbar, int var, int in, int opt) {
  cimq_conv_desc d;
  memset(&d, 0, sizeof(d));
  d.batch = B; d.in_channels = C; d.in_h = d.in_w = H; d.out_channels = O;
  d.kernel_h = d.kernel_w = k; d.stride_h = d.stride_w = s; d.pad_h = d.pad_w = k / 2; d.xbar = xbar;
  d.bits_w = d.bits_a = bits; d.bs_w = d.bs_a = 1; d.adc_bits = adc; d.adc_variant = var; d.input_kind = in;
  d.lsq_qp = (float)((1 << bits) - 1); d.options = opt;
  return d;
}

int main(int argc, char** argv) {
  if (argc < 2 || strcmp(argv[1], "--grid") != 0) {
    // bench.RESNET20's distinct w3a3 shapes: (C, O, H, stride)
    const int shapes[][4] = {{16, 16, 32, 1}, {16, 32, 32, 2}, {32, 32, 16, 1}, {32, 64, 16, 2}, {64, 64, 8, 1}};
    for (auto& s : shapes)
      for (int opt : {0, CIMQ_OPT_RECOMPUTE})
        probe(desc(256, s[0], s[1], s[2], s[3], 3, 3, 1.5f, 128, CIMQ_ADC_LIBRARY, CIMQ_INPUT_RAW_LSQ, opt));
    return 0;
  }
  for (int B : {1, 2, 4, 128})
    for (int C : {3, 8, 16, 32, 64})
      for (int O : {16, 32, 64, 128})
        for (int H : {1, 4, 8, 16, 32})
          for (int s : {1, 2})
            for (int k : {1, 3})
              for (int bits : {2, 3, 4, 8})
                for (float adc : {0.f, 1.f, 1.5f, 4.f})
                  for (int xbar : {64, 128})
                    for (int var : {CIMQ_ADC_LIBRARY, CIMQ_ADC_SHIFT_ROUND})
                      for (int in : {CIMQ_INPUT_XQ, CIMQ_INPUT_RAW_LSQ})
                        for (int opt : {0, CIMQ_OPT_RECOMPUTE, CIMQ_OPT_INFERENCE, CIMQ_OPT_RECOMPUTE | CIMQ_OPT_INFERENCE})
                          probe(desc(B, C, O, H, s, k, bits, adc, xbar, var, in, opt));
  return 0;
}
