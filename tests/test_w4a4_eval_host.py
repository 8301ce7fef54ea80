"""CPU: forward-only w4a4 layers in 1-bit slices on the stateless word-pair forward (host queries, no device work).

cimq_module_forward_form names the form of the forward kernel family the module entry points run: form[0] the state
format (Route::cst), form[1] whether the forward quantises the activation in its own row staging (Route::actq).  A
forward-only w4a4 descriptor answers (4, 1) on exactly the shapes whose training call runs the word pairs (4, 0: the
training forward keeps the prologue's pass over x); the shapes off the v7 plan, four slices of two bits and the shift
and stochastic ADCs keep the per-k family, (0, 0).  Nothing else moves: cimq_module_route and cimq_query_sizes of the
forward-only descriptors are the rows of tests/golden/w4a4_parent_table.json, column by column.

On a library from before the form both symbols are missing and every test here fails.
"""
import ctypes
import json

import pytest

import cim_quantization_amd._lib as L
from rect_cases import make_desc
from test_w4a4_routes_host import NDESC, TABLE, answer
from w4a4_cases import ADC_CASES, BAND_CASE, LITERAL_CASE, MODULE_CASES, UNMOVED, case_id, resnet20_3x3

INF = L.CIMQ_OPT_INFERENCE
EVAL_CASES = MODULE_CASES + ADC_CASES + [LITERAL_CASE, BAND_CASE]


@pytest.fixture(scope="module")
def lib():
    from cim_quantization_amd import build as cimq_build
    cimq_build.build(verbose=False)  # no-op when up to date (hipcc cross-compiles, no GPU needed)
    return L.load()


def _form(lib, d):
    f = (ctypes.c_int * 2)(-1, -1)
    assert lib.cimq_module_forward_form(ctypes.byref(d), f) == 0, lib.cimq_last_error()
    return (f[0], f[1])


def test_availability_symbol(lib):
    assert lib.cimq_w4a4_eval_abi() == 1
    assert {"cimq_w4a4_eval_abi", "cimq_module_forward_form"} <= set(L.EXPORTED_SYMBOLS)
    # no struct, call, size or route name moved: the ABI numbers are test_abi_host's
    assert L.module_forward_form(make_desc(L, MODULE_CASES[0], options=INF)) == (4, 1)


def test_refusals(lib):
    d = make_desc(L, MODULE_CASES[0], options=INF)
    f = (ctypes.c_int * 2)(-7, -7)
    assert lib.cimq_module_forward_form(None, f) == L.CIMQ_EINVAL
    assert lib.cimq_module_forward_form(ctypes.byref(d), None) == L.CIMQ_EINVAL
    assert lib.cimq_module_forward_form(None, None) == L.CIMQ_EINVAL
    # a bad descriptor: the usual errors, and form is left alone
    bad = make_desc(L, MODULE_CASES[0], options=64)
    assert lib.cimq_module_forward_form(ctypes.byref(bad), f) == L.CIMQ_EINVAL
    assert b"options" in lib.cimq_last_error()
    bad = make_desc(L, MODULE_CASES[0], options=INF)
    bad.xbar = 100
    assert lib.cimq_module_forward_form(ctypes.byref(bad), f) == L.CIMQ_EUNSUPPORTED
    # the Function form of a descriptor (x_q handed over) is not the module entry points'
    fn = make_desc(L, MODULE_CASES[0], options=INF)
    fn.input_kind = L.CIMQ_INPUT_XQ
    assert lib.cimq_module_forward_form(ctypes.byref(fn), f) == L.CIMQ_EINVAL
    assert (f[0], f[1]) == (-7, -7)


@pytest.mark.parametrize("c", EVAL_CASES, ids=case_id)
def test_forward_only_w4a4_runs_the_stateless_word_pairs(lib, c):
    assert (c["wb"], c["ab"], c["wbs"], c["abs"]) == (4, 4, 1, 1)
    assert _form(lib, make_desc(L, c, options=INF)) == (4, 1)
    assert _form(lib, make_desc(L, c, options=INF | L.CIMQ_OPT_RECOMPUTE)) == (4, 1)
    # the training forward writes the word pairs and keeps the prologue's pass over x
    assert _form(lib, make_desc(L, c)) == (4, 0)


@pytest.mark.parametrize("B", [256, 2])
def test_resnet20_3x3_layers(lib, B):
    cases = resnet20_3x3(B)
    assert len(cases) == 18
    for c in cases:
        assert _form(lib, make_desc(L, c, options=INF)) == (4, 1), case_id(c)
        assert _form(lib, make_desc(L, c)) == (4, 0), case_id(c)


@pytest.mark.parametrize("c", UNMOVED, ids=case_id)
def test_unmoved_keep_the_per_k_form(lib, c):
    """four slices of two bits, and the shapes off the v7 plan (O = 24 at 7 x 7, P = 192)"""
    assert _form(lib, make_desc(L, c, options=INF)) == (0, 0)
    assert _form(lib, make_desc(L, c)) == (0, 0)


@pytest.mark.parametrize("c", MODULE_CASES, ids=case_id)
def test_other_adc_variants_keep_the_per_k_form(lib, c):
    for variant in (L.CIMQ_ADC_SHIFT_ROUND, L.CIMQ_ADC_STOCHASTIC):
        assert _form(lib, make_desc(L, c, variant=variant, options=INF)) == (0, 0), variant
        assert _form(lib, make_desc(L, c, variant=variant)) == (0, 0), variant


def test_w3a3_is_unchanged(lib):
    c = dict(MODULE_CASES[0], wb=3, ab=3)
    assert _form(lib, make_desc(L, c, options=INF)) == (3, 1)
    assert _form(lib, make_desc(L, c)) == (3, 1)
    c2 = dict(MODULE_CASES[0], wb=2, ab=2)
    assert _form(lib, make_desc(L, c2, options=INF)) == (2, 1)


def test_routes_and_sizes_are_the_parents(lib):
    """every forward-only w4a4 row of the parent's table, on all nine answer columns -- the rows of the cases above
    among them -- and cimq_module_route still names (v3, none, none) where the form moved"""
    with open(TABLE) as f:
        rows = json.load(f)["rows"]
    fo = [r for r in rows if (r[NDESC - 1] & INF) and r[7:9] == [4, 1]]
    assert len(fo) >= 2 * len(EVAL_CASES)
    moved = 0
    for r in fo:
        assert answer(lib, r) == r[NDESC:NDESC + 9], r[:NDESC]
    for c in EVAL_CASES + resnet20_3x3(256) + resnet20_3x3(2):
        d = make_desc(L, c, options=INF)
        assert _form(lib, d) == (4, 1)
        assert tuple(L.ROUTE_NAMES[v] for v in L.module_route(d)) == ("v3", "none", "none")
        key = [c["B"], c["C"], c["O"], c["H"], c["W"], c["s"][0], c["xbar"], c["wb"], c["wbs"], c["adc"],
               L.CIMQ_ADC_LIBRARY, INF]
        assert any(r[:NDESC] == key for r in fo), key
        moved += 1
    assert moved == len(EVAL_CASES) + 36
