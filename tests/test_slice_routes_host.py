"""CPU: the kernels cimq_module_route names for the layers of slice_cases.py, whose weight or activation slices are
wider than one bit (host queries, no device work).  The plans keep such layers on the fast kernels, and
test_gpu_slices.py runs them there; this table fails if a later change gates a plan on a slice width of 1, where the
GPU cases would otherwise move to the general kernels without a word."""
import ctypes

import pytest

import cim_quantization_amd._lib as L
from rect_cases import make_desc, route_names
from slice_cases import (CODE_CASES, FORWARD_ONLY, MODULE_CASES, ROUTE_ONLY, SHIFT_CASES, case_id, codes_expected)


@pytest.fixture(scope="module")
def lib():
    from cim_quantization_amd import build as cimq_build
    cimq_build.build(verbose=False)  # no-op when up to date (hipcc cross-compiles, no GPU needed)
    return L.load()


@pytest.mark.parametrize("c", MODULE_CASES + ROUTE_ONLY, ids=case_id)
def test_module_route(lib, c):
    d = make_desc(L, c)
    assert (d.bs_w, d.bs_a, d.bits_w, d.bits_a) == (c["wbs"], c["abs"], c["wb"], c["ab"])
    assert d.lsq_qp == float(2 ** c["ab"] - 1)
    assert route_names(L, d) == c["route"]


@pytest.mark.parametrize("c", MODULE_CASES + ROUTE_ONLY, ids=case_id)
def test_forward_only_route_and_codes(lib, c):
    d = make_desc(L, c, options=L.CIMQ_OPT_INFERENCE)
    assert route_names(L, d) == (c["route"][0], "none", "none")
    assert L.codes_supported(d) == codes_expected(c)


@pytest.mark.parametrize("c,supported", SHIFT_CASES, ids=[case_id(c) for c, _ in SHIFT_CASES])
def test_shift_route(lib, c, supported):
    d = make_desc(L, c, variant=L.CIMQ_ADC_SHIFT_ROUND)
    assert lib.cimq_module_shift_supported(ctypes.byref(d)) == supported
    assert route_names(L, d) == c["route"]


def test_tables_reach_what_they_claim():
    """every fast backward family that admits a slice width other than 1, the dense path, and the general kernels;
    a slice wider than one bit in every case; the forward-only and code cases on the routes they name"""
    mods = MODULE_CASES + ROUTE_ONLY
    assert {c["route"] for c in mods} == {("general",) * 3, ("v3", "general", "general"), ("v3", "v7", "v7"),
                                           ("v3", "fused", "fused"), ("v3", "v7", "gw5"), ("v3", "gx5", "v7"),
                                           ("dense",) * 3}
    assert all(c["wbs"] > 1 or c["abs"] > 1 for c in mods + [c for c, _ in SHIFT_CASES])
    assert {MODULE_CASES[i]["route"][0] for i in FORWARD_ONLY} == {"v3", "dense"}
    assert all(codes_expected(MODULE_CASES[i]) == (True, True) for i in CODE_CASES)
    assert sorted(s for _, s in SHIFT_CASES) == [0, 1, 1] and SHIFT_CASES[0][1] == 0  # (general first)
