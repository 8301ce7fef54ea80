"""CIMQ_OPT_WIDE_BWD on the host: routes with and without the bit, sizes that do not move, the plan query."""
import json
import os

import pytest

import cim_quantization_amd._lib as L
from rect_cases import make_desc, route_names
from wide_bwd_cases import B4, CASES, REFUSED_64, WIDE_BWD
from test_wide_routes_host import NDESC, row_desc
from wide_cases import CASES as WCASES, UNMOVED, W6, W7, W8A, W8B, WIDE, case_id

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "wide_parent_table.json")


def _with_bit(c, extra=0):
    base = L.CIMQ_OPT_RECOMPUTE if c["recompute"] else 0
    return make_desc(L, c, options=base | L.CIMQ_OPT_WIDE_BWD | extra)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_routes_move_with_the_bit_only(c):
    assert L.load().cimq_wide_bwd_abi() == 1
    assert route_names(L, make_desc(L, c)) == WIDE
    assert route_names(L, _with_bit(c)) == WIDE_BWD
    assert route_names(L, _with_bit(c, L.CIMQ_OPT_INFERENCE)) == ("wide", "none", "none")
    assert L.module_wide_bwd_plan(make_desc(L, c))[0] == 1


# stride 2 (W6), 2-bit slices (W7) and the other ADC modes (W8a, W8b) stay on the general backward, as does every
# layer off the wide forward
@pytest.mark.parametrize("c", [WCASES[i] for i in (W6, W7, W8A, W8B)] + [REFUSED_64] + UNMOVED, ids=case_id)
def test_refused_layers_keep_their_routes(c):
    assert route_names(L, _with_bit(c)) == route_names(L, make_desc(L, c)) == c["route"]
    assert L.module_wide_bwd_plan(make_desc(L, c)) == (0, 0, 0, 0)


def test_sizes_do_not_move():
    """every row of the parent's table (wide_parent_table.json: sizes recorded from the library before the wide forward
    existed) answers the same five sizes with the bit added to its options"""
    with open(GOLDEN) as f:
        t = json.load(f)
    col = {n: i for i, n in enumerate(t["columns"])}
    sizes = [n for n, _ in L.Sizes._fields_]
    for row in t["rows"]:
        if row[col["rc"]] != 0:
            continue
        d = row_desc(row[:NDESC])
        d.options |= L.CIMQ_OPT_WIDE_BWD
        got = L.query_sizes(d)
        assert [getattr(got, n) for n in sizes] == [row[col[n]] for n in sizes], row[:NDESC]


def test_plan_of_b4_has_several_chunks():
    ok, chunks, bands, slabs = L.module_wide_bwd_plan(make_desc(L, CASES[B4]))
    assert ok == 1 and chunks >= 2 and bands >= 1 and slabs >= 1


def test_neighbouring_bits_stay_refused():
    """2 and 8 are no options (test_inference_host pins them on their own); nor beside the new bit, nor 32"""
    for bit in (2, 8, 32, 2 | L.CIMQ_OPT_WIDE_BWD, 8 | L.CIMQ_OPT_WIDE_BWD):
        with pytest.raises(L.CimqError, match="unknown options"):
            L.module_route(make_desc(L, CASES[0], options=bit))
