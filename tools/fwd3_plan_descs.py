#!/usr/bin/env python3
"""The descriptor list of tools/fwd3_plan_check.cpp, one per line on standard output: every descriptor of
tests/golden/route_table.json and every case dict of tests/rect_cases.py, slice_cases.py and w4a4_cases.py (module
descriptors: RAW_LSQ input), each with and without CIMQ_OPT_INFERENCE; the shift-ADC cases also as that variant.

    python tools/fwd3_plan_descs.py > descs.txt
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import cim_quantization_amd._lib as L  # noqa: E402  (constants and make_desc only: the library is not loaded)
import rect_cases  # noqa: E402
import slice_cases  # noqa: E402
import w4a4_cases  # noqa: E402

FIELDS = ["batch", "in_channels", "in_h", "in_w", "out_channels", "kernel_h", "kernel_w", "stride_h", "stride_w",
          "pad_h", "pad_w", "xbar", "bits_w", "bits_a", "bs_w", "bs_a", "adc_bits", "input_kind", "lsq_qp",
          "adc_variant", "options"]


def cases(mod):
    for v in vars(mod).values():
        for c in (v if isinstance(v, list) else [v]):
            if isinstance(c, dict) and "kh" in c:
                yield c


def main():
    descs = []
    with open(os.path.join(REPO, "tests", "golden", "route_table.json")) as f:
        for r in json.load(f)["rows"]:
            B, C, O, H, s, k, bits, adc, xbar, variant, opt = r[:11]
            descs.append(L.make_desc(B=B, C=C, H=H, W=H, O=O, KH=k, KW=k, stride=(s, s), padding=(k // 2, k // 2),
                                     xbar=xbar, bits_w=bits, bits_a=bits, bs_w=1, bs_a=1, adc_bits=adc,
                                     input_kind=L.CIMQ_INPUT_RAW_LSQ, lsq_qp=float(2 ** bits - 1), adc_variant=variant,
                                     options=opt))
    for mod in (rect_cases, slice_cases, w4a4_cases):
        shift = [id(c) for c in getattr(mod, "SHIFT_CASES", [])]
        for c in cases(mod):
            descs.append(rect_cases.make_desc(L, c))
            if id(c) in shift:
                descs.append(rect_cases.make_desc(L, c, variant=L.CIMQ_ADC_SHIFT_ROUND))
    seen = set()
    for d in descs:
        for opt in (d.options & ~L.CIMQ_OPT_INFERENCE, d.options | L.CIMQ_OPT_INFERENCE):
            d.options = opt
            line = " ".join(repr(getattr(d, f)) for f in FIELDS)
            if line not in seen:
                seen.add(line)
                print(line)


if __name__ == "__main__":
    main()
