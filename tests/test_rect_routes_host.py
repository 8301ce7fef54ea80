"""CPU: the kernels cimq_module_route names for the rectangular / anisotropic layers of rect_cases.py (host queries,
no device work).  test_gpu_rect.py runs the same layers on the device and asserts the same triples first, so a later
change of a plan gate cannot silently turn its fast-route cases into tests of the general kernels; this test lets the
CPU suite notice the drift too."""
import ctypes

import pytest

import cim_quantization_amd._lib as L
from rect_cases import BAND_CASE, FORWARD_ONLY, MODULE_CASES, SHIFT_CASES, case_id, make_desc, route_names


@pytest.fixture(scope="module")
def lib():
    from cim_quantization_amd import build as cimq_build
    cimq_build.build(verbose=False)  # no-op when up to date (hipcc cross-compiles, no GPU needed)
    return L.load()


@pytest.mark.parametrize("c", MODULE_CASES + [BAND_CASE], ids=case_id)
def test_module_route(lib, c):
    assert route_names(L, make_desc(L, c)) == c["route"]


@pytest.mark.parametrize("idx", FORWARD_ONLY)
def test_forward_only_route(lib, idx):
    c = MODULE_CASES[idx]
    opt = (L.CIMQ_OPT_RECOMPUTE if c["recompute"] else 0) | L.CIMQ_OPT_INFERENCE
    assert route_names(L, make_desc(L, c, options=opt)) == (c["route"][0], "none", "none")


@pytest.mark.parametrize("c", SHIFT_CASES, ids=case_id)
def test_shift_route(lib, c):
    d = make_desc(L, c, variant=L.CIMQ_ADC_SHIFT_ROUND)
    assert lib.cimq_module_shift_supported(ctypes.byref(d)) == 1
    assert route_names(L, d) == c["route"]


def test_routes_cover_every_backward_family():
    """the table reaches each backward kernel family the module path has but the dense one (1 x 1 images only)"""
    got = {c["route"][1] for c in MODULE_CASES} | {c["route"][2] for c in MODULE_CASES}
    assert got == {"general", "v7", "gx5", "gw5", "r6", "fused", "c1"}
    assert {c["route"][0] for c in MODULE_CASES} == {"general", "v3", "fwd5"}
