"""CPU: the routes and sizes of w4a4 layers in 1-bit slices (host queries, no device work).

Such a layer trains on the compact-state backward -- cimq_module_route names (v3, v7, v7) -- where the v7 plan takes
its shape; its forward-only calls, the shift and stochastic ADCs, four slices of two bits and the shapes off the plan
stay where they were.  tests/golden/w4a4_parent_table.json holds what the library of the parent commit (ea2c129, which
ran these layers on the general backward) answered for a fixed list of descriptors: forward-only rows must match it on
every column, training rows on ctx_bytes, module_ctx_bytes, wprep_bytes and fwd_workspace_bytes (the 8-byte state words
fill the region the per-k words had).  bwd_workspace_bytes may move with the backward, so the table holds both sides'.
To record it again:

    CIMQ_LIB_PATH=<the parent's libcimq.so> python tests/test_w4a4_routes_host.py parent tests/golden/w4a4_parent_table.json
    python tests/test_w4a4_routes_host.py new tests/golden/w4a4_parent_table.json
"""
import ctypes
import json
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pytest

import cim_quantization_amd._lib as L
from rect_cases import make_desc, route_names
from w4a4_cases import (ADC_CASES, BAND_CASE, FORWARD_ONLY, FUNCTION_CASES, LITERAL_CASE, MODULE_CASES, UNMOVED, V7,
                        case_id, resnet20_3x3)

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "w4a4_parent_table.json")
KEYS = ["B", "C", "O", "H", "W", "s", "xbar", "wb", "wbs", "adc"]
COLUMNS = KEYS + ["adc_variant", "options", "rc", "fwd", "gx", "gw", "ctx_bytes", "fwd_workspace_bytes",
                  "bwd_workspace_bytes", "wprep_bytes", "module_ctx_bytes", "bwd_workspace_bytes_new"]
NDESC = len(KEYS) + 2
INF = L.CIMQ_OPT_INFERENCE

GPU_CASES = MODULE_CASES + ADC_CASES + FUNCTION_CASES + [LITERAL_CASE, BAND_CASE]


def _cases():
    return GPU_CASES + UNMOVED + resnet20_3x3(256) + resnet20_3x3(2)


def descriptors():
    """every case as a training and a forward-only descriptor; the ternary-ADC ones under the shift and the
    stochastic ADC too (square 3 x 3 kernels, pad 1: the cases' own)"""
    rows = []
    for c in _cases():
        key = tuple(c["s"][0] if k == "s" else c[k] for k in KEYS)
        rows.append(key + (L.CIMQ_ADC_LIBRARY, 0))
        rows.append(key + (L.CIMQ_ADC_LIBRARY, INF))
        if c["adc"] == 1.5:
            rows.append(key + (L.CIMQ_ADC_SHIFT_ROUND, 0))
            rows.append(key + (L.CIMQ_ADC_SHIFT_ROUND, INF))
            rows.append(key + (L.CIMQ_ADC_STOCHASTIC, 0))
    return list(dict.fromkeys(rows))


def row_desc(row):
    B, C, O, H, W, s, xbar, wb, wbs, adc, variant, opt = row[:NDESC]
    return L.make_desc(B=B, C=C, H=H, W=W, O=O, KH=3, KW=3, stride=(s, s), padding=(1, 1), xbar=xbar, bits_w=wb,
                       bits_a=wb, bs_w=wbs, bs_a=wbs, adc_bits=adc, input_kind=L.CIMQ_INPUT_RAW_LSQ,
                       lsq_qp=float(2 ** wb - 1), adc_variant=variant, options=opt)


def answer(lib, row):
    """[rc, fwd, gx, gw] of cimq_module_route and the five cimq_sizes fields for one descriptor row"""
    d = row_desc(row)
    r = (ctypes.c_int * 3)()
    rc = lib.cimq_module_route(ctypes.byref(d), r)
    s = L.Sizes()
    assert lib.cimq_query_sizes(ctypes.byref(d), ctypes.byref(s)) == 0, lib.cimq_last_error()
    return [rc, r[0], r[1], r[2], s.ctx_bytes, s.fwd_workspace_bytes, s.bwd_workspace_bytes, s.wprep_bytes,
            s.module_ctx_bytes]


@pytest.fixture(scope="module")
def lib():
    from cim_quantization_amd import build as cimq_build
    cimq_build.build(verbose=False)  # no-op when up to date (hipcc cross-compiles, no GPU needed)
    return L.load()


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        t = json.load(f)
    assert t["columns"] == COLUMNS
    return t["rows"]


@pytest.mark.parametrize("c", GPU_CASES, ids=case_id)
def test_gpu_cases_train_on_v7(lib, c):
    d = make_desc(L, c)
    assert (d.bits_w, d.bits_a, d.bs_w, d.bs_a) == (4, 4, 1, 1)
    assert c["route"] == V7 and route_names(L, d) == V7
    assert route_names(L, make_desc(L, c, options=INF)) == ("v3", "none", "none")


@pytest.mark.parametrize("B", [256, 2])
def test_resnet20_3x3_layers_train_on_v7(lib, B):
    cases = resnet20_3x3(B)
    assert len(cases) == 18 and len({(c["C"], c["O"], c["H"], c["s"]) for c in cases}) == 5
    for c in cases:
        assert route_names(L, make_desc(L, c)) == V7, case_id(c)


@pytest.mark.parametrize("c", UNMOVED, ids=case_id)
def test_unmoved_routes(lib, c):
    assert route_names(L, make_desc(L, c)) == c["route"]


@pytest.mark.parametrize("c", MODULE_CASES, ids=case_id)
def test_other_adc_variants_keep_the_general_backward(lib, c):
    """the shift ADC's statistics kernel takes two or three slices only (cimq_module_shift_supported answers 0 and
    the module runs its torch composition); the stochastic ADC is the general kernels' throughout"""
    d = make_desc(L, c, variant=L.CIMQ_ADC_SHIFT_ROUND)
    assert lib.cimq_module_shift_supported(ctypes.byref(d)) == 0
    assert route_names(L, d)[1:] == ("general", "general")
    d = make_desc(L, c, variant=L.CIMQ_ADC_STOCHASTIC)
    assert route_names(L, d)[1:] == ("general", "general")


def test_table_is_the_parents(table):
    """the fixture holds the descriptor list above, and was recorded where these layers ran the general backward"""
    assert [tuple(r[:NDESC]) for r in table] == descriptors()
    assert os.path.getsize(TABLE) < 200 * 1024
    names = lambda r: tuple(L.ROUTE_NAMES[v] for v in r[NDESC + 1:NDESC + 4])  # noqa: E731
    lib_training = [r for r in table if r[NDESC - 2] == L.CIMQ_ADC_LIBRARY and r[NDESC - 1] == 0 and r[7:9] == [4, 1]]
    assert len(lib_training) >= 15 and all(names(r)[1:] == ("general", "general") for r in lib_training)


def test_sizes_against_the_parent_table(lib, table):
    bad = []
    for r in table:
        want, got = r[NDESC:NDESC + 9], answer(lib, r)
        if r[NDESC - 1] & INF:
            ok = got == want  # forward only: nothing moves
        else:
            # rc; ctx_bytes, fwd_workspace_bytes, wprep_bytes, module_ctx_bytes as the parent's; the backward
            # workspace as recorded from this library
            ok = got[0] == want[0] == 0 and [got[i] for i in (4, 5, 7, 8)] == [want[i] for i in (4, 5, 7, 8)] and \
                got[6] == r[NDESC + 9]
            if tuple(got[1:4]) != tuple(want[1:4]):  # a route moved: a w4a4 layer onto v7, nothing else
                ok = ok and r[7:9] == [4, 1] and r[NDESC - 2] == L.CIMQ_ADC_LIBRARY and \
                    tuple(L.ROUTE_NAMES[v] for v in got[1:4]) == V7
        if not ok:
            bad.append((r[:NDESC], want, r[NDESC + 9], got))
    assert not bad, (len(bad), bad[:5])


def test_forward_only_indices():
    assert [MODULE_CASES[i]["O"] for i in FORWARD_ONLY] == [16, 32, 64]


if __name__ == "__main__":
    mode, path = sys.argv[1], sys.argv[2]
    lib_ = L.load()
    if mode == "parent":
        rows_ = [list(row) + answer(lib_, row) + [None] for row in descriptors()]
    else:
        with open(path) as f_:
            rows_ = json.load(f_)["rows"]
        assert [tuple(r[:NDESC]) for r in rows_] == descriptors()
        for r in rows_:
            r[NDESC + 9] = answer(lib_, r)[6]
    with open(path, "w") as f_:
        f_.write('{"columns": %s,\n "rows": [\n' % json.dumps(COLUMNS))
        f_.write(",\n".join("  " + json.dumps(r) for r in rows_))
        f_.write("\n ]}\n")
    print(f"{len(rows_)} rows ({mode}) from {L.LIB_PATH}")
