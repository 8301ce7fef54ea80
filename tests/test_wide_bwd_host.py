"""CIMQ_OPT_WIDE_BWD on the host: routes with and without the bit, sizes that do not move, the plan query."""
import json
import os

import pytest

import cim_quantization_amd._lib as L
from rect_cases import make_desc, route_names
from wide_bwd_cases import B4, BATCH_CASES, CASES, REFUSED_64, WIDE_BWD, batch_plan, stage_images
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


@pytest.mark.parametrize("c", BATCH_CASES, ids=case_id)
def test_batch_cases_leave_the_trivial_plan(c):
    """N1 .. N4 exist for the batch-dependent launch parameters: several input rows a grad_x band and several stages a
    grad_w workgroup, in the counts the table records (a later plan change must not turn them back into RB = 1 /
    nstage = 1 cases without this test noticing)"""
    assert route_names(L, make_desc(L, c)) == WIDE
    assert route_names(L, _with_bit(c)) == WIDE_BWD
    ok, chunks, bands, slabs = L.module_wide_bwd_plan(make_desc(L, c))
    stages, nstage = batch_plan(c, max(slabs, 1))
    print(f"{case_id(c)}: (ok, chunks, bands, slabs) = {(ok, chunks, bands, slabs)}, ceil(H / bands) = "
          f"{-(-c['H'] // max(bands, 1))}, {stages} stages, nstage = {nstage}")
    assert ok == 1 and (bands, slabs) == c["plan"]
    assert -(-c["H"] // bands) > 1 and nstage > 1


def test_batch_cases_reach_what_they_name():
    """the right-hand column of the issue's table, from the plan's answers"""
    rb = lambda c: -(-c["H"] // c["plan"][0])  # noqa: E731
    n1, n2, n3, n4 = BATCH_CASES
    # N1: three ring steps a band (RB + 1 = 9 output rows, four a step), a chunk is two whole images
    assert rb(n1) == 8 and batch_plan(n1, n1["plan"][1]) == (256, 4) and stage_images(n1, 4, 1) == [2, 3]
    # N2: odd nstage, so every other chunk starts mid-image; the last chunk is one stage
    assert rb(n2) == 4 and batch_plan(n2, n2["plan"][1]) == (160, 3)
    assert stage_images(n2, 3, 0) == [0, 1] and stage_images(n2, 3, 1) == [1, 2] and 160 - 53 * 3 == 1
    # N3: a partial last band (two bands at B * ceil(12 / 8) = 256: RB = 8, rows 8 + 4), three stages an image
    assert n3["B"] * n3["plan"][0] == 256 and n3["H"] % 8 == 4 and batch_plan(n3, n3["plan"][1]) == (384, 6)
    # N4: the w4a4 word pair with two steps a band (RB + 1 = 5 output rows, four a step) and two stages a workgroup
    assert n4["wb"] == 4 and rb(n4) == 4 and batch_plan(n4, n4["plan"][1]) == (128, 2)


def test_neighbouring_bits_stay_refused():
    """2 and 8 are no options (test_inference_host pins them on their own); nor beside the new bit, nor 32"""
    for bit in (2, 8, 32, 2 | L.CIMQ_OPT_WIDE_BWD, 8 | L.CIMQ_OPT_WIDE_BWD):
        with pytest.raises(L.CimqError, match="unknown options"):
            L.module_route(make_desc(L, CASES[0], options=bit))
