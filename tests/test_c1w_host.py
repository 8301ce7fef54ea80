"""CIMQ_OPT_WIDE_BWD on the w8a8 first conv beyond 16 output channels, on the host: routes with and without the bit,
the plan query, sizes that do not move."""
import pytest

import cim_quantization_amd._lib as L
from c1w_cases import C1W, CASES, GENERAL, GROUPS, UNMOVED, routes
from rect_cases import case_id, make_desc, route_names

BIT = L.CIMQ_OPT_WIDE_BWD


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_routes_move_with_the_bit_only(c):
    assert L.load().cimq_c1w_abi() == 1
    # (the forward is out of the bit's reach: cim_fwd_v3_kernel where 256 % O == 0, else the general kernel)
    want = routes(c)
    assert want[1:] == C1W[1:] and (want[0] == "v3") == (256 % c["O"] == 0)
    assert route_names(L, make_desc(L, c)) == (want[0],) + GENERAL[1:]
    assert route_names(L, make_desc(L, c, options=BIT)) == want
    assert route_names(L, make_desc(L, c, options=BIT | L.CIMQ_OPT_INFERENCE)) == (want[0], "none", "none")
    ok, groups, per_group, steps = L.module_c1w_plan(make_desc(L, c))
    blocks = c["O"] // 16
    assert ok == 1 and steps == c["H"] * c["W"] // 128
    assert 1 <= groups <= 9 and (groups - 1) * per_group < blocks <= groups * per_group
    if c is CASES[GROUPS]:
        assert groups >= 2


@pytest.mark.parametrize("c", UNMOVED, ids=case_id)
def test_refused_layers_keep_their_routes(c):
    want = route_names(L, make_desc(L, c))
    assert c["route"] in (None, want) and "c1w" not in want
    assert route_names(L, make_desc(L, c, options=BIT)) == want
    assert L.module_c1w_plan(make_desc(L, c)) == (0, 0, 0, 0)


@pytest.mark.parametrize("variant", ["CIMQ_ADC_SHIFT_ROUND", "CIMQ_ADC_STOCHASTIC"])
def test_other_adc_variants_keep_their_routes(variant):
    c, v = CASES[0], getattr(L, variant)
    assert route_names(L, make_desc(L, c, variant=v, options=BIT)) == route_names(L, make_desc(L, c, variant=v))
    assert L.module_c1w_plan(make_desc(L, c, variant=v)) == (0, 0, 0, 0)


@pytest.mark.parametrize("c", CASES + UNMOVED, ids=case_id)
def test_sizes_do_not_move(c):
    off, on = L.query_sizes(make_desc(L, c)), L.query_sizes(make_desc(L, c, options=BIT))
    for name, _ in L.Sizes._fields_:
        assert getattr(on, name) == getattr(off, name), name
