"""Weight and activation slices wider than one bit (wbitslice / abitslice != 1): the case tables shared by the host
route test (test_slice_routes_host.py) and the GPU parity tests (test_gpu_slices.py).  Plain data built with
rect_cases.case; no fixtures, no device work.  ``wb`` / ``ab`` are the bit widths and ``wbs`` / ``abs`` the slice
widths, so a side has int(bits / slice) slices: 5 bits in 2-bit slices are two slices that drop the top bit."""
from rect_cases import case


def sl(B, C, O, H, W, wb, ab, wbs, abs_, **kw):
    return case(B, C, O, H, W, wb=wb, ab=ab, wbs=wbs, abs=abs_, **kw)


def case_id(c):
    t = "%dx%dto%d_%dx%d_k%d_s%d_w%da%d_bs%d%d_adc%s_x%d" % (
        c["B"], c["C"], c["O"], c["H"], c["W"], c["kh"], c["s"][0], c["wb"], c["ab"], c["wbs"], c["abs"], c["adc"],
        c["xbar"])
    return t + ("_signed" if c["signed"] else "")


GEN = ("general", "general", "general")
V7 = ("v3", "v7", "v7")
FUSED = ("v3", "fused", "fused")
DENSE = ("dense", "dense", "dense")

# ---- the Function path (get_cim_output_signed, [B, P, O]): the general-route case first ----
FUNCTION_CASES = [
    sl(2, 16, 24, 7, 7, 4, 4, 2, 2, xbar=64),
    sl(2, 16, 16, 16, 16, 4, 4, 2, 2),
    sl(2, 16, 16, 16, 16, 4, 4, 2, 2, xbar=64),
    sl(2, 16, 32, 16, 16, 4, 4, 2, 2, s=2),
    sl(2, 16, 16, 16, 16, 4, 4, 2, 2, adc=4),
    # sign ADC: power-of-two scales, so that sign(ps) at ps = 0 has no fp32 residue to follow
    sl(2, 16, 16, 16, 16, 4, 4, 2, 2, adc=1, sa=0.125, sw=0.0625),
    sl(2, 16, 16, 16, 16, 6, 6, 2, 2),
    sl(2, 16, 16, 32, 32, 6, 3, 2, 1),
    sl(2, 16, 16, 32, 32, 3, 6, 1, 2),
    sl(2, 16, 16, 16, 16, 5, 5, 2, 2),
    sl(2, 16, 16, 16, 16, 8, 8, 2, 2),
    sl(2, 3, 16, 16, 16, 8, 8, 2, 2, signed=1),
    sl(2, 16, 16, 16, 16, 8, 8, 4, 4),
    # the dense path (1 x 1 kernels on 1 x 1 images): 4 slice pairs; 16 slice pairs with a partial last tile
    sl(128, 64, 64, 1, 1, 4, 4, 2, 2, k=1, p=0),
    sl(128, 80, 64, 1, 1, 8, 8, 2, 2, k=1, p=0, xbar=64),
]

# 4-bit slices reach |ps| > 2048, where the reference's fp16 store rounds: power-of-two scales keep every slice an
# exact integer, and C = 32 (with activations that are not zeroed, test_gpu_slices.py) raises the share of such sums
FP16_CASE = sl(2, 32, 16, 16, 16, 8, 8, 4, 4, sa=0.03125, sw=0.015625)

# ---- the module path (Conv2dLSQCiM, steady state) with the (forward, grad_x, grad_w) kernels cimq_module_route
# must name for each: the general-backward case first ----
MODULE_CASES = [
    sl(2, 16, 16, 16, 16, 8, 8, 2, 2, route=("v3", "general", "general")),   # 16 slice pairs of 2-bit slices
    sl(2, 16, 16, 16, 16, 4, 4, 2, 2, route=V7),
    sl(2, 16, 16, 16, 16, 6, 6, 2, 2, route=V7),                            # 9 slice pairs
    sl(2, 16, 16, 16, 16, 5, 5, 2, 2, route=V7),                            # two slices, the top bit dropped
    sl(2, 16, 16, 16, 16, 8, 8, 4, 4, route=V7),                            # 4-bit slices
    sl(2, 16, 32, 16, 16, 4, 4, 2, 2, s=2, route=V7),                       # stride 2
    sl(2, 16, 64, 16, 16, 4, 4, 2, 2, route=FUSED),
    sl(2, 64, 64, 8, 8, 4, 4, 2, 2, route=FUSED),
    sl(2, 16, 64, 16, 16, 6, 6, 2, 2, route=FUSED),
    sl(2, 16, 16, 32, 32, 6, 3, 2, 1, route=("v3", "v7", "gw5")),           # gw5 gates the activation side alone
    sl(2, 16, 16, 32, 32, 3, 6, 1, 2, route=("v3", "gx5", "v7")),           # gx5 gates the weight side alone
    sl(128, 64, 64, 1, 1, 4, 4, 2, 2, k=1, p=0, route=DENSE),
]

# further layers whose route the host test pins (the route table of the change that added these tests)
ROUTE_ONLY = [
    sl(2, 16, 16, 16, 16, 4, 4, 2, 2, xbar=64, route=V7),
    sl(2, 16, 16, 8, 16, 4, 4, 2, 2, route=V7),
    sl(2, 16, 16, 8, 8, 4, 4, 2, 2, route=V7),
    sl(2, 16, 64, 8, 16, 4, 4, 2, 2, xbar=64, route=FUSED),
    sl(2, 16, 16, 32, 32, 6, 6, 2, 2, route=V7),
    sl(2, 16, 16, 16, 16, 6, 3, 2, 1, route=("v3", "v7", "gw5")),
    sl(2, 3, 16, 16, 16, 8, 8, 2, 2, signed=1, route=("v3", "general", "general")),
    sl(2, 16, 16, 16, 16, 4, 4, 2, 2, adc=4, route=V7),
    sl(128, 64, 64, 1, 1, 8, 8, 2, 2, k=1, p=0, route=DENSE),
    sl(2, 16, 24, 7, 7, 4, 4, 2, 2, xbar=64, route=GEN),
]



def codes_expected(c):
    """cimq_module_codes_supported's (in, out) answers under CIMQ_OPT_INFERENCE: codes go in wherever Qp + 1 fits a
    byte (not at 8 activation bits), and come out of every forward but the dense one"""
    return c["ab"] < 8, c["route"][0] != "dense"


# the forward-only modes and the fused evaluation run on these module cases (by index)
FORWARD_ONLY = [1, 6, 9, 10, 11]

# activation codes in and out (by index): 2-bit activation slices at 4 and at 6 bits
CODE_CASES = [1, 10]

# Conv2dLSQCiM(adc_shift=True): (case, cimq_module_shift_supported's answer).  xbar 128 with 2-bit slices on both
# sides has psmax = 128 * 4 * 4 = 2048, the largest the shift path admits; O = 24 is just off the path
SHIFT_CASES = [
    (sl(2, 16, 24, 16, 16, 4, 4, 2, 2, route=GEN), 0),
    (sl(2, 16, 16, 16, 16, 4, 4, 2, 2, route=V7), 1),
    (sl(2, 16, 16, 16, 16, 4, 4, 2, 2, xbar=64, route=V7), 1),
]
