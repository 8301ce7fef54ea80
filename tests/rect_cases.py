"""Rectangular images and anisotropic kernel / stride / padding: the case tables shared by the host route test
(test_rect_routes_host.py) and the GPU parity tests (test_gpu_rect.py).  Plain data and two small helpers; no
fixtures, no device work."""


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def case(B, C, O, H, W, k=3, s=1, p=1, bits=3, adc=1.5, xbar=128, signed=0, recompute=False, route=None, **extra):
    """one layer; k / s / p are ints (both axes) or (h, w) pairs.  ``bits`` sets both widths with 1-bit slices;
    ``wb`` / ``ab`` / ``wbs`` / ``abs`` among ``extra`` override them one by one (slice_cases.py)"""
    kh, kw = _pair(k)
    d = dict(B=B, C=C, O=O, H=H, W=W, kh=kh, kw=kw, s=_pair(s), p=_pair(p), wb=bits, ab=bits, wbs=1, abs=1, adc=adc,
             xbar=xbar, signed=signed, recompute=recompute, route=route)
    d.update(extra)
    return d


def case_id(c):
    t = "%dx%dto%d_%dx%d_k%dx%d_s%d%d_p%d%d_w%d_adc%s_x%d" % (
        c["B"], c["C"], c["O"], c["H"], c["W"], c["kh"], c["kw"], c["s"][0], c["s"][1], c["p"][0], c["p"][1], c["wb"],
        c["adc"], c["xbar"])
    return t + ("_rec" if c["recompute"] else "")


def out_hw(c):
    return ((c["H"] + 2 * c["p"][0] - c["kh"]) // c["s"][0] + 1, (c["W"] + 2 * c["p"][1] - c["kw"]) // c["s"][1] + 1)


# ---- the Function path (get_cim_output_signed, [B, P, O]): general-route cases first ----
FUNCTION_CASES = [
    # xbar 64, odd P, O no multiple of 16: the general kernels everywhere
    case(2, 16, 24, 5, 7, xbar=64),
    case(2, 16, 24, 7, 5, k=(3, 2), s=(2, 1), p=(1, 0), xbar=64),
    # one step off the dense path's H = W = 1 gate
    case(128, 64, 64, 1, 2, k=1, p=0, xbar=64),
    case(64, 64, 64, 2, 1, k=1, p=0, xbar=64),
    # anisotropic kernel / stride / padding: the fast forward, the general backward
    case(2, 16, 16, 8, 16, k=(1, 3), p=(0, 1)),
    case(2, 16, 16, 8, 16, k=(3, 1), p=(1, 0)),
    case(2, 16, 16, 8, 32, s=(1, 2)),
    case(2, 16, 16, 16, 16, s=(2, 1)),
    case(2, 16, 16, 10, 16, p=(0, 1)),
    # the other slice counts and ADC modes on a rectangle
    case(2, 16, 16, 8, 16, bits=2, xbar=64),
    case(2, 16, 16, 8, 16, adc=4),
    case(2, 16, 16, 8, 16, adc=1, sa=0.125, sw=0.0625),
    # the fast forward with the compact-state backward
    case(2, 16, 16, 8, 32),
    case(2, 16, 16, 12, 32),
    case(2, 16, 16, 32, 8),
    case(2, 16, 16, 4, 64),
    case(2, 16, 16, 16, 64),
    # the fused backward
    case(2, 64, 64, 4, 16),
    case(2, 64, 64, 2, 32),
    # stride-2 grad_x
    case(2, 16, 32, 16, 32, s=2),
    case(2, 16, 32, 32, 16, s=2),
    # w8a8, signed: the first-conv backward
    case(2, 3, 16, 8, 32, bits=8, signed=1),
    case(2, 3, 16, 16, 8, bits=8, signed=1),
]

# ---- the module path (Conv2dLSQCiM, steady state) with the (forward, grad_x, grad_w) kernels cimq_module_route
# must name for each: general-route cases first ----
MODULE_CASES = [
    case(2, 16, 24, 7, 5, k=(3, 2), s=(2, 1), p=(1, 0), xbar=64, route=("general", "general", "general")),
    case(2, 16, 16, 6, 32, route=("v3", "general", "general")),            # P = 192 fails the 128-pixel gates
    case(2, 16, 16, 8, 16, k=(1, 3), p=(0, 1), route=("v3", "general", "general")),  # NCHW forward, [B,P,O] backward
    case(2, 16, 16, 8, 32, s=(1, 2), route=("v3", "general", "general")),
    case(2, 16, 16, 8, 16, bits=2, xbar=64, route=("v3", "v7", "v7")),
    case(2, 16, 16, 8, 16, adc=4, route=("v3", "v7", "gw5")),
    case(2, 16, 16, 8, 32, route=("fwd5", "gx5", "gw5")),                  # H != W on the one-launch gx5 + gw5 pair
    case(2, 16, 16, 12, 32, route=("fwd5", "gx5", "gw5")),                 # three m-tiles per image
    case(3, 16, 16, 8, 32, route=("fwd5", "gx5", "gw5")),                  # odd batch
    case(4, 32, 32, 4, 16, route=("fwd5", "gx5", "gw5")),                  # P = 64: two whole images per m-tile
    case(2, 16, 16, 8, 32, recompute=True, route=("fwd5", "r6", "r6")),    # the recompute backward
    case(2, 16, 16, 32, 8, route=("fwd5", "v7", "gw5")),                   # tall and narrow: 16 rows per m-tile
    case(2, 16, 16, 4, 64, route=("fwd5", "v7", "v7")),                    # W = 64: one row per 64-pixel step
    case(2, 16, 16, 16, 64, route=("fwd5", "v7", "v7")),                   # W = 64, many steps
    case(2, 64, 64, 4, 16, route=("fwd5", "fused", "fused")),              # the fused kernel with R = 4
    case(2, 64, 64, 2, 32, route=("fwd5", "fused", "fused")),              # ... with R = 2
    case(2, 16, 64, 8, 32, xbar=64, route=("fwd5", "fused", "fused")),     # ... several steps, grad_w in LDS
    case(2, 16, 32, 16, 32, s=2, route=("fwd5", "v7", "gw5")),             # stride 2, Ho != Wo
    case(2, 16, 32, 32, 16, s=2, route=("fwd5", "v7", "gw5")),
    case(2, 3, 16, 8, 32, bits=8, signed=1, route=("v3", "c1", "c1")),     # the first-conv kernel, two steps
    case(2, 3, 16, 16, 8, bits=8, signed=1, route=("v3", "c1", "c1")),     # ... one step of 16 rows
]

# 8-row grad_x bands at stride 1 need B * ceil(H / 8) >= 256: H = 12 gives an 8-row and a partial 4-row band
BAND_CASE = case(128, 32, 32, 12, 32, route=("fwd5", "v7", "gw5"))

# the forward-only modes run on these module cases (by index)
FORWARD_ONLY = [6, 12, 15, 19, 0]

# Conv2dLSQCiM(adc_shift=True): cimq_module_shift_supported answers 1
SHIFT_CASES = [
    case(2, 16, 16, 8, 16, bits=2, xbar=64, route=("v3", "v7", "v7")),
    case(2, 16, 16, 8, 32, route=("v3", "v7", "v7")),
]


def make_desc(L, c, variant=None, options=None):
    """the module entry points' descriptor of a case (RAW_LSQ input)"""
    opt = (L.CIMQ_OPT_RECOMPUTE if c["recompute"] else 0) if options is None else options
    return L.make_desc(B=c["B"], C=c["C"], H=c["H"], W=c["W"], O=c["O"], KH=c["kh"], KW=c["kw"], stride=c["s"],
                       padding=c["p"], xbar=c["xbar"], bits_w=c["wb"], bits_a=c["ab"], bs_w=c["wbs"], bs_a=c["abs"],
                       adc_bits=c["adc"], input_kind=L.CIMQ_INPUT_RAW_LSQ, lsq_qp=float(2 ** c["ab"] - 1),
                       adc_variant=L.CIMQ_ADC_LIBRARY if variant is None else variant, options=opt)


def route_names(L, desc):
    return tuple(L.ROUTE_NAMES[v] for v in L.module_route(desc))
