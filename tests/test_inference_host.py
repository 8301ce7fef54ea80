"""CPU: the forward-only mode of the C ABI (CIMQ_OPT_INFERENCE, ABI 15) as the host sees it -- the option
bits, the sizes cimq_query_sizes reports under it, the route query, and the refusal of every entry point
that has no forward-only form.  Host queries only: no device work."""
import ctypes

import pytest

import cim_quantization_amd._lib as L
from cim_quantization_amd import build as cimq_build

INF = 4  # CIMQ_OPT_INFERENCE (the value is part of the ABI: 2 must stay refused)

# the shapes the GPU tests (test_gpu_inference.py) run, with the forward route each must take
#        B,  C,  O,   H, stride, bits, xbar, adc, kernel, pad, route
CASES = {
    "l1": (1, 16, 16, 32, 1, 3, 128, 1.5, 3, 1, "fwd5"),
    "l2": (1, 32, 32, 16, 1, 3, 128, 1.5, 3, 1, "fwd5"),
    "l2s2": (1, 16, 32, 32, 2, 3, 128, 1.5, 3, 1, "fwd5"),
    "l3": (2, 64, 64, 8, 1, 3, 128, 1.5, 3, 1, "fwd5"),
    "conv1": (2, 3, 16, 32, 1, 8, 64, 1.5, 3, 1, "v3"),
    "w2a2": (2, 16, 16, 16, 1, 2, 128, 1.5, 3, 1, "v3"),
    "adc6": (1, 16, 16, 32, 1, 3, 128, 6, 3, 1, "v3"),
    "c48": (1, 48, 48, 16, 1, 3, 128, 1.5, 3, 1, "general"),
    "dense": (128, 256, 256, 1, 1, 4, 128, 1.5, 1, 0, "dense"),
    "shift": (2, 16, 16, 8, 1, 3, 128, 1.5, 3, 1, "v3"),
}


def case_desc(name, options=0, **kw):
    B, C, O, H, s, nb, xbar, adc, k, p, _ = CASES[name]
    args = dict(B=B, C=C, H=H, W=H, O=O, KH=k, KW=k, stride=(s, s), padding=(p, p), xbar=xbar, bits_w=nb, bits_a=nb,
                bs_w=1, bs_a=1, adc_bits=adc, input_kind=L.CIMQ_INPUT_RAW_LSQ, lsq_qp=float(2 ** nb - 1),
                adc_variant=L.CIMQ_ADC_SHIFT_ROUND if name == "shift" else L.CIMQ_ADC_LIBRARY, options=options)
    args.update(kw)
    return L.make_desc(**args)


def resnet20_descs(options):
    import bench
    for name, c, o, h, s, nb in bench.RESNET20:
        yield name, L.make_desc(B=256, C=c, H=h, W=h, O=o, KH=3, KW=3, stride=(s, s), padding=(1, 1), xbar=bench.XBAR,
                                bits_w=nb, bits_a=nb, bs_w=1, bs_a=1, adc_bits=bench.ADC,
                                input_kind=L.CIMQ_INPUT_RAW_LSQ, lsq_qp=float(2 ** nb - 1), options=options)


def all_descs(options):
    for name in CASES:
        yield name, case_desc(name, options)
    yield from resnet20_descs(options)


@pytest.fixture(scope="module")
def lib():
    cimq_build.build(verbose=False)
    return L.load()


def _sizes(lib, d):
    s = L.Sizes()
    assert lib.cimq_query_sizes(ctypes.byref(d), ctypes.byref(s)) == 0, lib.cimq_last_error()
    return s


def _route(lib, d):
    r = (ctypes.c_int * 3)()
    assert lib.cimq_module_route(ctypes.byref(d), r) == 0, lib.cimq_last_error()
    return tuple(r)


def test_option_bits(lib):
    assert L.CIMQ_OPT_INFERENCE == INF and L.ABI_VERSION >= 15
    for opt in (INF, INF | L.CIMQ_OPT_RECOMPUTE):
        d = case_desc("l1", opt)
        _sizes(lib, d)
        _route(lib, d)
    for opt in (2, 8):
        d = case_desc("l1", opt)
        assert lib.cimq_query_sizes(ctypes.byref(d), ctypes.byref(L.Sizes())) == L.CIMQ_EINVAL
        assert b"unknown options" in lib.cimq_last_error()
        assert lib.cimq_module_route(ctypes.byref(d), (ctypes.c_int * 3)()) == L.CIMQ_EINVAL


def test_case_routes(lib):
    """every case takes the forward route the GPU tests mean to exercise, and the shift case is one the fused
    shift entry points take"""
    for name, c in CASES.items():
        assert L.ROUTE_NAMES[_route(lib, case_desc(name))[0]] == c[-1], name
    assert lib.cimq_module_shift_supported(ctypes.byref(case_desc("shift"))) == 1
    assert lib.cimq_module_shift_supported(ctypes.byref(case_desc("shift", INF))) == 1


def test_sizes(lib):
    for (name, d0), (_, d1) in zip(all_descs(0), all_descs(INF)):
        s0, s1 = _sizes(lib, d0), _sizes(lib, d1)
        B, C, H, W, O = d0.batch, d0.in_channels, d0.in_h, d0.in_w, d0.out_channels
        K = C * d0.kernel_h * d0.kernel_w
        T = -(-K // d0.xbar)
        Ho = (H + 2 * d0.pad_h - d0.kernel_h) // d0.stride_h + 1
        Wo = (W + 2 * d0.pad_w - d0.kernel_w) // d0.stride_w + 1
        M, nin = B * Ho * Wo, B * C * H * W
        nbp = 4 if d0.bits_a // d0.bs_a <= 4 else 8
        assert s1.ctx_bytes == s1.module_ctx_bytes, name
        # the state region and the backward slice words, both lower bounds of ctx_layout_compute's
        assert s0.ctx_bytes - s1.ctx_bytes >= 4 * T * M * O + nbp * nin, name
        assert s1.bwd_workspace_bytes == 0, name
        general = d0.adc_variant == L.CIMQ_ADC_LIBRARY and L.ROUTE_NAMES[_route(lib, d0)[0]] == "general"
        assert s1.fwd_workspace_bytes <= 64 * 1024 + (4 * M * O if general else 0), name
        assert s1.wprep_bytes == s0.wprep_bytes, name
    # with the recompute bit next to it: the same forward-only sizes, around the weight-side layout that bit has
    # without the inference bit (wprep_bytes: the recompute backward's operand keeps its place, unwritten)
    s5 = _sizes(lib, case_desc("l1", INF | L.CIMQ_OPT_RECOMPUTE))
    s1 = _sizes(lib, case_desc("l1", INF))
    assert s5.wprep_bytes == _sizes(lib, case_desc("l1", L.CIMQ_OPT_RECOMPUTE)).wprep_bytes
    assert (s5.ctx_bytes - s5.wprep_bytes, s5.fwd_workspace_bytes, s5.bwd_workspace_bytes) == \
        (s1.ctx_bytes - s1.wprep_bytes, s1.fwd_workspace_bytes, 0)
    assert s5.ctx_bytes == s5.module_ctx_bytes


def test_route(lib):
    assert L.ROUTE_NAMES[L.CIMQ_ROUTE_NONE] == "none" and L.CIMQ_ROUTE_NONE == 10
    for (name, d0), (_, d1) in zip(all_descs(0), all_descs(INF)):
        if d0.adc_variant != L.CIMQ_ADC_LIBRARY:
            continue  # (cimq_module_route answers for the library ADC)
        r0, r1 = _route(lib, d0), _route(lib, d1)
        assert r1[0] == r0[0], name
        assert r1[1] == r1[2] == L.CIMQ_ROUTE_NONE, name
        assert L.CIMQ_ROUTE_NONE not in r0, name


REFUSED = [("cimq_backward", 14), ("cimq_module_backward", 17), ("cimq_module_backward_chain", 18),
           ("cimq_module_backward_tail", 10), ("cimq_module_backward_params", 11), ("cimq_module_shift_backward", 19),
           ("cimq_shift_forward", 12), ("cimq_shift_backward", 16), ("cimq_alpha_init", 10),
           ("cimq_debug_partial_sums", 12), ("cimq_debug_state_codes", 4), ("cimq_debug_recompute_codes", 7)]


@pytest.mark.parametrize("entry,nargs", REFUSED)
def test_refusals(lib, entry, nargs):
    """the entry points with no forward-only form refuse an inference descriptor before they look at any
    pointer: every other argument is null"""
    for name in ("l1", "shift"):
        d = case_desc(name, INF)
        fn = getattr(lib, entry)
        assert len(fn.argtypes) == nargs + 1
        lib.cimq_module_route(None, None)  # leaves another message behind
        assert fn(ctypes.byref(d), *([None] * nargs)) == L.CIMQ_EINVAL, entry
        assert b"CIMQ_OPT_INFERENCE" in lib.cimq_last_error(), (entry, lib.cimq_last_error())
    # ... and still answer as before for a training descriptor (all-null pointers: their own messages)
    assert getattr(lib, entry)(ctypes.byref(case_desc("l1")), *([None] * nargs)) != 0
    assert b"CIMQ_OPT_INFERENCE" not in lib.cimq_last_error()


def test_accepting_entry_points_validate_as_before(lib):
    """the four accepting entry points take the descriptor (null pointers are their usual error, not the option's)"""
    d = case_desc("l1", INF)
    for entry, nargs in (("cimq_forward", 11), ("cimq_module_forward", 12)):
        assert getattr(lib, entry)(ctypes.byref(d), *([None] * nargs)) == L.CIMQ_EINVAL
        assert b"CIMQ_OPT_INFERENCE" not in lib.cimq_last_error()
    assert lib.cimq_module_shift_forward(ctypes.byref(case_desc("shift", INF)), *([None] * 13)) == L.CIMQ_EINVAL
    assert b"CIMQ_OPT_INFERENCE" not in lib.cimq_last_error()
