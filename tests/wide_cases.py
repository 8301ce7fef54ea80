"""Module layers whose input channels do not fit the fast forward's whole-C LDS patch (C >= 128: VGG7's 3 x 3 layers)
on the channel-chunked forward, cim_fwd_wide_kernel: the case tables shared by the host route test
(test_wide_routes_host.py) and the GPU tests (test_gpu_wide.py).  Plain data built with rect_cases.case; no fixtures,
no device work.  The GPU tests pin the step sizes at the 97 % quantiles of x and |w| (test_gpu_rect._module_data,
step="quantile") and assert the coverage conditions on the module oracle's values: every slice pair has 5-95 % nonzero
ADC codes, at least 1 % of the activations sit at Qp and the weights reach both clamp ends."""
from rect_cases import case

WIDE = ("wide", "general", "general")
GENERAL = ("general", "general", "general")
V3_GENERAL = ("v3", "general", "general")


def wd(B, C, O, H, W, **kw):
    kw.setdefault("route", WIDE)
    return case(B, C, O, H, W, **kw)


def case_id(c):
    t = "%dx%dto%d_%dx%d_s%d_w%da%d_bs%d%d_adc%s_x%d" % (
        c["B"], c["C"], c["O"], c["H"], c["W"], c["s"][0], c["wb"], c["ab"], c["wbs"], c["abs"], c["adc"], c["xbar"])
    return t


# W1 .. W8 (W9 is W1 with an all-equal alpha_cim: the literal flag).  The 128-channel cases are 16 x 16 and not 8 x 8:
# at 8 x 8 such a layer passes v3_plan (its V3::NT is exactly 32, its patch 51 KB) and keeps the fast forward, which
# UNMOVED holds it to; from 16 x 16 on, or from 144 channels, the whole-C plan refuses and the wide one takes over.
CASES = [
    wd(2, 128, 128, 16, 16),                                # W1: T = 9, four m-tiles an image
    wd(2, 256, 128, 4, 16, bits=4),                         # W2: w4a4, rectangular, Wo = 16
    wd(2, 128, 256, 16, 16, bits=2, xbar=64),               # W3: four output groups, one K-step
    wd(2, 512, 512, 8, 8),                                  # W4: T = 36, at least two channel chunks
    wd(2, 144, 160, 8, 8),                                  # W5: 16-row last tile, partial last output group
    wd(2, 128, 128, 16, 16, s=2),                           # W6: stride 2
    wd(2, 128, 128, 16, 16, wb=4, ab=4, wbs=2, abs=2),      # W7: 4 / 4 in 2-bit slices, the runtime slice path
    wd(2, 128, 128, 16, 16, adc=4),                         # W8a: a multi-bit ADC, the literal path
    wd(2, 128, 128, 16, 16, adc=1, sa=0.125, sw=0.0625),    # W8b: the sign ADC, the literal path
]
W1, W2, W3, W4, W5, W6, W7, W8A, W8B = range(9)
TERNARY = [W1, W2, W3, W4, W5, W6, W7]  # the ternary ADC: coverage is asserted on the oracle's codes
BACKWARD = [W1, W5]                      # the general backward behind the wide forward, against the oracle
FUSED = [W1, W3, W5]                     # forward_fused


def vgg7_wide(B):
    """VGG7's five 3 x 3 layers from 128 input channels up (CIFAR, 32 x 32 input), w3a3"""
    return [wd(B, 128, 128, 32, 32), wd(B, 128, 256, 16, 16), wd(B, 256, 256, 16, 16), wd(B, 256, 512, 8, 8),
            wd(B, 512, 512, 8, 8)]


# ---- routes that must stay where they are ----
UNMOVED = [
    wd(2, 128, 128, 16, 16, bits=8, route=GENERAL),   # w8a8: eight slices a side
    wd(2, 128, 128, 8, 8, route=V3_GENERAL),           # 128 -> 128 at 8 x 8 fits the whole-C patch: as before
    wd(2, 64, 64, 32, 32, route=GENERAL),              # C = 64 at 32 x 32: below the plan's 128 channels
    wd(2, 16, 16, 6, 32, bits=4, route=V3_GENERAL),    # P = 192 (w4a4_cases.UNMOVED): the fast forward as before
    wd(2, 128, 128, 6, 16, route=GENERAL),             # 128 channels, P = 96: no whole 64-pixel m-tiles per image
    wd(2, 128, 128, 12, 12, route=GENERAL),            # 128 channels, Wo = 12 divides no 64-pixel m-tile
    wd(2, 136, 128, 8, 8, route=GENERAL),              # C no multiple of 16
    wd(2, 128, 72, 8, 8, route=GENERAL),               # O no multiple of 16
]
