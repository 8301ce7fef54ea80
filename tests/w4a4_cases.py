"""w4a4 layers in 1-bit slices (four slices a side, 16 slice pairs) on the compact-state backward: the case tables
shared by the host route test (test_w4a4_routes_host.py) and the GPU tests (test_gpu_w4a4.py).  Plain data built with
rect_cases.case(..., bits=4); no fixtures, no device work."""
from rect_cases import case

V7 = ("v3", "v7", "v7")
V3_GENERAL = ("v3", "general", "general")
GENERAL = ("general", "general", "general")


def w4(B, C, O, H, W, **kw):
    kw.setdefault("route", V7)
    return case(B, C, O, H, W, bits=4, **kw)


def case_id(c):
    t = "%dx%dto%d_%dx%d_s%d_w%da%d_bs%d%d_adc%s_x%d" % (
        c["B"], c["C"], c["O"], c["H"], c["W"], c["s"][0], c["wb"], c["ab"], c["wbs"], c["abs"], c["adc"], c["xbar"])
    return t + ("_signed" if c["signed"] else "")


# ---- the module path (Conv2dLSQCiM, steady state): every case trains on (v3, v7, v7) ----
MODULE_CASES = [
    w4(2, 16, 16, 16, 16),             # T = 2, the last tile has 16 rows
    w4(2, 16, 16, 16, 16, xbar=64),    # T = 3
    w4(2, 16, 32, 16, 16, s=2),        # Wo = 8, one 128-pixel stage, two output blocks
    w4(2, 16, 64, 16, 16),             # four output blocks; the fused gate refuses four slices
    w4(2, 64, 64, 8, 8),               # four input blocks, T = 5, whole-image stages
    w4(2, 16, 16, 32, 32),             # Wo = 32: NPART 1, two column segments
    w4(2, 32, 32, 16, 16),             # C = 32, two output blocks
]

# the other ADC modes on shape 1 (the forward's per-pair write path): a multi-bit ADC (no alpha_cim, pass bits only)
# and the sign ADC, with power-of-two scales as the slice suite's sign case has them
ADC_CASES = [
    w4(2, 16, 16, 16, 16, xbar=64, adc=4),
    w4(2, 16, 16, 16, 16, xbar=64, adc=1, sa=0.125, sw=0.0625),
]

# the Function path ([B, P, O]): shapes 0 and 2 (shape 0 also with one binary_mask entry altered)
FUNCTION_CASES = [MODULE_CASES[0], MODULE_CASES[2]]

# test_gpu_alpha_equal's all-equal alpha_cim at 4 bits: the literal flag
LITERAL_CASE = w4(2, 16, 16, 16, 16, xbar=64)

# test_gpu_rect's partial last grad_x band (an 8-row and a 4-row band) at 4 bits
BAND_CASE = w4(128, 32, 32, 12, 32)

# the forward-only contract runs on these module cases (by index); codes and the two-layer plan on the first
FORWARD_ONLY = [0, 2, 4]

# ---- routes that must stay where they are ----
UNMOVED = [
    # 8 / 8 bits in 2-bit slices: four slices a side too, but no 1-bit ones
    case(2, 16, 16, 16, 16, wb=8, ab=8, wbs=2, abs=2, route=V3_GENERAL),
    case(2, 3, 16, 16, 16, wb=8, ab=8, wbs=2, abs=2, signed=1, route=V3_GENERAL),
    w4(2, 16, 24, 7, 7, xbar=64, route=GENERAL),   # O = 24 at 7 x 7: off every fast plan
    w4(2, 16, 16, 6, 32, route=V3_GENERAL),        # P = 192 fails the 128-pixel gates
]


def resnet20_3x3(B):
    """ResNet-20's 18 3 x 3 CiM convs (bench.RESNET20 without the w8a8 first conv) at 4 bits"""
    import bench
    return [w4(B, c, o, h, h, s=s, xbar=bench.XBAR, adc=bench.ADC) for name, c, o, h, s, _ in bench.RESNET20
            if name != "conv1"]
