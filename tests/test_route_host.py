"""CPU: which kernels the module entry points run (cimq_module_route) and what they need (cimq_query_sizes), for a
fixed list of descriptors, against tests/golden/route_table.json (host queries, no device work).

The table was recorded from the library of commit 2a27fe6 -- the parent of the change that moved the choice of kernels
into one host-side Route -- so the test pins that the routes and every size came through it unchanged.  To record it
again from a revision whose answers are to be kept:

    CIMQ_LIB_PATH=<that revision's libcimq.so> python tests/test_route_host.py tests/golden/route_table.json
"""
import ctypes
import json
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pytest

import cim_quantization_amd._lib as L

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "route_table.json")
COLUMNS = ["B", "C", "O", "H", "stride", "k", "bits", "adc_bits", "xbar", "adc_variant", "options",
           "rc", "fwd", "gx", "gw", "ctx_bytes", "fwd_workspace_bytes", "bwd_workspace_bytes", "wprep_bytes",
           "module_ctx_bytes"]
NDESC = 11
REC, INF = L.CIMQ_OPT_RECOMPUTE, L.CIMQ_OPT_INFERENCE

# the smallest descriptor of every route the module entry points take (1-bit slices, pad k / 2, RAW_LSQ input):
# (B, C, O, H, stride, k, bits, adc_bits, xbar, options) -> (forward, grad_x, grad_w)
SMALLEST = [
    ((1, 16, 16, 32, 1, 3, 3, 1.5, 128, 0), ("fwd5", "gx5", "gw5")),
    ((1, 16, 16, 32, 1, 3, 3, 1.5, 128, REC), ("fwd5", "r6", "r6")),
    ((1, 16, 16, 16, 1, 3, 3, 1.5, 128, 0), ("fwd5", "v7", "gw5")),
    ((1, 16, 16, 16, 1, 3, 3, 1.5, 64, 0), ("fwd5", "v7", "v7")),
    ((1, 16, 64, 16, 1, 3, 3, 1.5, 64, 0), ("fwd5", "fused", "fused")),
    ((1, 3, 16, 16, 1, 3, 8, 0, 64, 0), ("v3", "c1", "c1")),
    ((1, 3, 64, 16, 1, 3, 2, 0, 64, 0), ("v3", "fused", "fused")),
    ((1, 16, 16, 32, 1, 3, 3, 0, 128, 0), ("v3", "gx5", "gw5")),
    ((1, 16, 16, 16, 1, 3, 3, 0, 128, 0), ("v3", "v7", "gw5")),
    ((1, 3, 16, 16, 1, 3, 2, 0, 64, 0), ("v3", "v7", "v7")),
    ((1, 3, 16, 8, 1, 1, 2, 0, 64, 0), ("v3", "general", "general")),
    ((128, 16, 64, 1, 1, 1, 2, 1.5, 64, 0), ("dense", "dense", "dense")),
    ((1, 3, 16, 1, 1, 1, 2, 0, 64, 0), ("general", "general", "general")),
]


def descriptors():
    """the recorded list: every SMALLEST row, its forward-only form and (w2a2) its shift-ADC form; every layer of the
    benchmark's ResNet-20; a grid of 3 x 3 layers; 1 x 1 images around the dense path"""
    import bench
    rows = []
    for (B, C, O, H, s, k, bits, adc, xbar, opt), _ in SMALLEST:
        rows.append((B, C, O, H, s, k, bits, adc, xbar, L.CIMQ_ADC_LIBRARY, opt))
        rows.append((B, C, O, H, s, k, bits, adc, xbar, L.CIMQ_ADC_LIBRARY, opt | INF))
        if bits == 2:  # (the shift ADC needs adc_bits >= 1)
            rows.append((B, C, O, H, s, k, bits, 1.5, xbar, L.CIMQ_ADC_SHIFT_ROUND, opt))
    for _, c, o, h, s, nb in bench.RESNET20:
        for opt in (0, REC, INF):
            rows.append((256, c, o, h, s, 3, nb, bench.ADC, bench.XBAR, L.CIMQ_ADC_LIBRARY, opt))
    for B in (2, 128):
        for C in (3, 16):
            for O in (16, 64):
                for H in (8, 32):
                    for s in (1, 2):
                        for bits in (2, 3, 8):
                            for adc in (0, 1.5):
                                for xbar in (64, 128):
                                    for opt in (0, REC):
                                        rows.append((B, C, O, H, s, 3, bits, adc, xbar, L.CIMQ_ADC_LIBRARY, opt))
    for C in (16, 64):
        for O in (64, 128):
            for bits in (2, 3, 4):
                for xbar in (64, 128):
                    rows.append((128, C, O, 1, 1, 1, bits, 1.5, xbar, L.CIMQ_ADC_LIBRARY, 0))
    return list(dict.fromkeys(rows))


def make_desc(row):
    B, C, O, H, s, k, bits, adc, xbar, variant, opt = row[:NDESC]
    return L.make_desc(B=B, C=C, H=H, W=H, O=O, KH=k, KW=k, stride=(s, s), padding=(k // 2, k // 2), xbar=xbar,
                       bits_w=bits, bits_a=bits, bs_w=1, bs_a=1, adc_bits=adc, input_kind=L.CIMQ_INPUT_RAW_LSQ,
                       lsq_qp=float(2 ** bits - 1), adc_variant=variant, options=opt)


def answer(lib, row):
    """[rc, fwd, gx, gw] of cimq_module_route and the five cimq_sizes fields for one descriptor row"""
    d = make_desc(row)
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


def test_table_covers_every_route(table):
    """the fixture holds the descriptor list above, within its size limit, and every route triple the module path has"""
    assert [tuple(r[:NDESC]) for r in table] == descriptors()
    assert len(table) <= 1500 and os.path.getsize(TABLE) < 200 * 1024
    got = {tuple(L.ROUTE_NAMES[v] for v in r[NDESC + 1:NDESC + 4]) for r in table}
    want = {t for _, t in SMALLEST} | {(f, "none", "none") for f in ("general", "v3", "fwd5", "dense")}
    assert got == want


def test_smallest_descriptor_of_each_route(lib):
    for row, want in SMALLEST:
        full = row[:9] + (L.CIMQ_ADC_LIBRARY, row[9])
        a = answer(lib, full)
        assert a[0] == 0 and tuple(L.ROUTE_NAMES[v] for v in a[1:4]) == want, (row, a[:4])
        a = answer(lib, full[:10] + (row[9] | INF,))
        assert a[0] == 0 and tuple(L.ROUTE_NAMES[v] for v in a[1:4]) == (want[0], "none", "none"), (row, a[:4])


def test_routes_and_sizes_match_the_recorded_table(lib, table):
    """every row: the route, all five sizes, and return code 0 -- cimq_module_route refuses a descriptor whose Function
    and module forms (output layout flag off / on) do not share every weight-side ctx offset, every workspace offset
    and the workspace size"""
    bad = [(r[:NDESC], r[NDESC:], answer(lib, r)) for r in table if answer(lib, r) != r[NDESC:] or r[NDESC] != 0]
    assert not bad, (len(bad), bad[:5])


if __name__ == "__main__":
    lib_ = L.load()
    rows_ = [list(row) + answer(lib_, row) for row in descriptors()]
    with open(sys.argv[1], "w") as f_:
        f_.write('{"columns": %s,\n "rows": [\n' % json.dumps(COLUMNS))
        f_.write(",\n".join("  " + json.dumps(r) for r in rows_))
        f_.write("\n ]}\n")
    print(f"{len(rows_)} rows from {L.LIB_PATH}")
