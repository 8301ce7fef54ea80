// fwd3_plan_check.cpp -- what v3_plan answers for a list of descriptors, and the dynamic LDS launch_fwd_v3 asks for,
// as one text line per descriptor: compile it once against each of two trees' cimq_host.h and diff the outputs.
// Host code only (make_geo and v3_plan are host functions; nothing touches a device).
//
//   hipcc -x hip --cuda-host-only -std=c++17 -I <tree>/cim_quantization_amd/csrc tools/fwd3_plan_check.cpp -o check
//   python tools/fwd3_plan_descs.py | ./check
//
// Columns: the descriptor, then with the output layout flag off and on (the Function's [B, P, O] and the module's
// NCHW): ok, fwd_res, lds_fwd, obm, and launch_fwd_v3's bytes without and with the fused activation quantiser.
#include "cimq_host.h"

int main() {
  using namespace cimq;
  cimq_conv_desc d;
  memset(&d, 0, sizeof(d));
  double adc, qp;
  while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %lf %d %lf %d %d", &d.batch, &d.in_channels, &d.in_h,
               &d.in_w, &d.out_channels, &d.kernel_h, &d.kernel_w, &d.stride_h, &d.stride_w, &d.pad_h, &d.pad_w,
               &d.xbar, &d.bits_w, &d.bits_a, &d.bs_w, &d.bs_a, &adc, &d.input_kind, &qp, &d.adc_variant,
               &d.options) == 21) {
    d.adc_bits = (float)adc;
    d.lsq_qp = (float)qp;
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %g %d %g %d %d :", d.batch, d.in_channels, d.in_h, d.in_w,
           d.out_channels, d.kernel_h, d.kernel_w, d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.xbar, d.bits_w, d.bits_a,
           d.bs_w, d.bs_a, adc, d.input_kind, qp, d.adc_variant, d.options);
    Geo g;
    if (make_geo(&d, &g) != CIMQ_OK) {
      printf(" refused\n");
      continue;
    }
    for (int onchw = 0; onchw < 2; ++onchw) {
      g.onchw = onchw;
      const Plan3 p = v3_plan(g);
      printf(" ok %d fwd_res %d lds_fwd %zu obm %d launch %zu %zu", (int)p.ok, p.v.fwd_res, p.lds_fwd, p.v.obm,
             p.lds_fwd, p.lds_fwd + (size_t)kActLutMax * 2 * 4);
    }
    printf("\n");
  }
  return 0;
}
