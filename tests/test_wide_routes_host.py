"""CPU: the routes, plans and sizes of module layers on the channel-chunked forward (host queries, no device work).

A 3 x 3 module layer from 128 input channels up, whose channels do not fit the fast forward's whole-C LDS patch, runs
cim_fwd_wide_kernel: cimq_module_route names (wide, general, general), and (wide, none, none) forward only.  The
shift and stochastic ADCs, w8a8 and the shapes off the plan stay where they were.  tests/golden/wide_parent_table.json
holds what the library of the parent commit (ca85026, which ran these layers on the general forward) answered for a
fixed list of descriptors: every size column must match it on every row, and so must every route but the forward's of
the rows the plan takes.  To record it again:

    CIMQ_LIB_PATH=<the parent's libcimq.so> python tests/test_wide_routes_host.py tests/golden/wide_parent_table.json
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
from wide_cases import CASES, UNMOVED, W1, W3, W4, WIDE, case_id, vgg7_wide, wd

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide_parent_table.json")
GOLDEN_VGG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "harness_vggsmall_cim_state.json")
KEYS = ["B", "C", "O", "H", "W", "s", "xbar", "wb", "ab", "wbs", "abs", "adc"]
COLUMNS = KEYS + ["adc_variant", "options", "rc", "fwd", "gx", "gw", "ctx_bytes", "fwd_workspace_bytes",
                  "bwd_workspace_bytes", "wprep_bytes", "module_ctx_bytes"]
NDESC = len(KEYS) + 2
INF = L.CIMQ_OPT_INFERENCE


def _cases():
    return CASES + vgg7_wide(256) + vgg7_wide(2) + UNMOVED


def descriptors():
    """every case as a training and a forward-only descriptor; the ternary-ADC ones under the shift and the stochastic
    ADC too (square 3 x 3 kernels, pad 1: the cases' own)"""
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
    B, C, O, H, W, s, xbar, wb, ab, wbs, abs_, adc, variant, opt = row[:NDESC]
    return L.make_desc(B=B, C=C, H=H, W=W, O=O, KH=3, KW=3, stride=(s, s), padding=(1, 1), xbar=xbar, bits_w=wb,
                       bits_a=ab, bs_w=wbs, bs_a=abs_, adc_bits=adc, input_kind=L.CIMQ_INPUT_RAW_LSQ,
                       lsq_qp=float(2 ** ab - 1), adc_variant=variant, options=opt)


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


def test_symbols(lib):
    assert lib.cimq_wide_abi() == 1
    assert hasattr(lib, "cimq_module_wide_plan")
    assert L.CIMQ_ROUTE_WIDE == 11 and L.ROUTE_NAMES[11] == "wide"
    assert "cimq_wide_abi" in L.EXPORTED_SYMBOLS and "cimq_module_wide_plan" in L.EXPORTED_SYMBOLS
    # the other availability numbers are what they were
    assert (lib.cimq_abi_version(), lib.cimq_abi_minor()) == (16, 1)
    assert lib.cimq_w4a4_eval_abi() == 1 and lib.cimq_net_abi() == 1


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_cases_run_the_wide_forward(lib, c):
    assert c["route"] == WIDE and route_names(L, make_desc(L, c)) == WIDE
    d = make_desc(L, c, options=INF)
    assert route_names(L, d) == ("wide", "none", "none")
    # a forward-only call quantises in the kernel's row staging; the family's state format is the per-k one's number
    assert L.module_forward_form(d) == (0, 1) and L.module_forward_form(make_desc(L, c)) == (0, 0)
    ok, chunks, groups, tiles = L.module_wide_plan(make_desc(L, c))
    assert ok == 1 and chunks >= 1 and tiles == -(-c["C"] * 9 // c["xbar"])
    assert groups == -(-c["O"] // 64)
    assert L.module_wide_plan(d) == (ok, chunks, groups, tiles)


def test_plans_of_the_table(lib):
    assert L.module_wide_plan(make_desc(L, CASES[W4]))[1] >= 2  # 512 channels: several channel chunks
    assert L.module_wide_plan(make_desc(L, CASES[W3]))[2] >= 2  # 256 output channels: several output groups
    assert L.module_wide_plan(make_desc(L, CASES[W4]))[3] == 36


@pytest.mark.parametrize("B", [256, 2])
def test_vgg7_wide_layers(lib, B):
    cases = vgg7_wide(B)
    assert [(c["C"], c["O"], c["H"]) for c in cases] == [(128, 128, 32), (128, 256, 16), (256, 256, 16), (256, 512, 8),
                                                         (512, 512, 8)]
    for c in cases:
        assert route_names(L, make_desc(L, c)) == WIDE, case_id(c)
        assert route_names(L, make_desc(L, c, options=INF)) == ("wide", "none", "none"), case_id(c)
        assert L.module_wide_plan(make_desc(L, c))[0] == 1


@pytest.mark.parametrize("c", UNMOVED, ids=case_id)
def test_unmoved_routes(lib, c):
    assert route_names(L, make_desc(L, c)) == c["route"]
    assert L.module_wide_plan(make_desc(L, c)) == (0, 0, 0, 0)


@pytest.mark.parametrize("c", [c for c in CASES if c["adc"] == 1.5], ids=case_id)
def test_other_adc_variants_keep_the_general_forward(lib, c):
    for variant in (L.CIMQ_ADC_SHIFT_ROUND, L.CIMQ_ADC_STOCHASTIC):
        assert route_names(L, make_desc(L, c, variant=variant)) == ("general", "general", "general")
        assert L.module_wide_plan(make_desc(L, c, variant=variant)) == (0, 0, 0, 0)
    assert route_names(L, make_desc(L, c, variant=L.CIMQ_ADC_SHIFT_ROUND, options=INF)) == ("general", "none", "none")


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_codes_are_refused(lib, c):
    d = make_desc(L, c, options=INF)
    i, o = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.cimq_module_codes_supported(ctypes.byref(d), ctypes.byref(i), ctypes.byref(o)) == 0
    assert (i.value, o.value) == (0, 0)


# ---- refusals, decided on the host before anything is dereferenced or launched: made-up device addresses ----
def _wide_desc(C, O, H, B=2, bits=3):
    return make_desc(L, wd(B, C, O, H, H, bits=bits), options=INF)


def test_forward_codes_refused(lib):
    """cimq_module_forward_codes on a wide layer with codes on either side: CIMQ_EUNSUPPORTED"""
    from test_codes_host import XQ, _call, _io, _refused
    d = make_desc(L, CASES[W1], options=INF)
    _refused(lib, _call(lib, d, _io()), b"wide route", L.CIMQ_EUNSUPPORTED)                            # out_codes
    _refused(lib, _call(lib, d, _io(x_codes=XQ, out_codes=None)), b"wide route", L.CIMQ_EUNSUPPORTED)  # x_codes
    _refused(lib, _call(lib, d, _io(x_codes=XQ)), b"wide route", L.CIMQ_EUNSUPPORTED)                  # both


def _net_plan(descs, n_slots):
    from test_net_host import Plan
    p = Plan(names=("l1",) * len(descs), n_slots=n_slots)
    p.descs = list(descs)
    d0 = descs[0]
    p.shape = (d0.batch, d0.in_channels, d0.in_h, d0.in_w)
    return p


def _net_refused(lib, p, word):
    """cimq_net_forward and cimq_net_sizes answer the same"""
    assert p.forward(lib) == L.CIMQ_EUNSUPPORTED, lib.cimq_last_error()
    msg = lib.cimq_last_error()
    assert b"cimq_net_forward" in msg and word in msg, msg
    assert p.sizes(lib)[0] == L.CIMQ_EUNSUPPORTED and word in lib.cimq_last_error()


def test_net_plans_with_a_wide_layer(lib):
    """a cimq_net_forward plan holding a wide layer: accepted with fp32 edges and a whole-tensor residual, refused
    with codes in, codes out or a residual view"""
    narrow, wide = _wide_desc(16, 128, 16), _wide_desc(128, 128, 16)
    assert route_names(L, narrow)[0] in ("v3", "fwd5") and route_names(L, wide)[0] == "wide"
    # fp32 edges, the second wide layer adding the first one's output: cimq_net_sizes accepts it
    p = _net_plan([narrow, wide, wide], 3)
    p.layers[2].res_slot = 1
    rc, fb, cb, ws = p.sizes(lib)
    assert rc == 0 and fb == [2 * 128 * 16 * 16 * 4] * 3 and cb == [0, 0, 0], lib.cimq_last_error()
    assert ws == max(L.query_sizes(d).fwd_workspace_bytes for d in p.descs)
    # codes into a wide layer (the producer, on the fast forward, could write them)
    p = _net_plan([narrow, wide], 2)
    p.layers[0].out_mode, p.layers[0].consumer, p.layers[1].in_codes = 3, 1, 1
    _net_refused(lib, p, b"the wide route takes no x_codes")
    # codes out of a wide layer
    p = _net_plan([narrow, wide, wide], 3)
    p.layers[1].out_mode, p.layers[1].consumer, p.layers[2].in_codes = 3, 2, 1
    _net_refused(lib, p, b"the wide route writes no out_codes")
    # a residual view: 64 source channels into 128 (layer 0 writes them, layer 1 reads x itself)
    src = _wide_desc(128, 64, 16)
    p = _net_plan([src, wide], 2)
    p.layers[1].in_slot, p.layers[1].res_slot, p.layers[1].res_c0 = -1, 0, 32
    _net_refused(lib, p, b"the wide route reads no residual view")
    # ... and at stride 2: a 32 x 32 source over the 16 x 16 output
    src2 = _wide_desc(128, 128, 32)
    down = make_desc(L, wd(2, 128, 128, 32, 32, s=2), options=INF)
    p = _net_plan([src2, down, wide], 3)
    p.layers[2].res_slot, p.layers[2].res_stride = 0, 2
    _net_refused(lib, p, b"layer 2: the wide route reads no residual view")


def test_table_is_the_parents(table):
    """the fixture holds the descriptor list above, and was recorded where these layers ran the general forward"""
    assert [tuple(r[:NDESC]) for r in table] == descriptors()
    assert os.path.getsize(TABLE) < 200 * 1024
    assert all(r[NDESC + 1] != L.CIMQ_ROUTE_WIDE for r in table)
    general = [r for r in table if r[NDESC + 1] == 0]
    assert len(general) >= 2 * (len(CASES) + 9)


def test_sizes_and_routes_against_the_parent_table(lib, table):
    bad, moved = [], 0
    for r in table:
        want, got = r[NDESC:NDESC + 9], answer(lib, r)
        ok = got[0] == want[0] and got[4:] == want[4:] and got[2:4] == want[2:4]  # rc, every size, both backward roles
        if got[1] != want[1]:  # the forward moved: the library ADC from the general kernel onto the wide one only
            ok = ok and r[NDESC - 2] == L.CIMQ_ADC_LIBRARY and want[1] == 0 and got[1] == L.CIMQ_ROUTE_WIDE
            moved += 1
        if not ok:
            bad.append((r[:NDESC], want, got))
    assert not bad, (len(bad), bad[:5])
    # the nine cases and VGG7's five shapes at two batch sizes (W4 is one of them), as training and forward-only rows
    wide = {tuple(c["s"][0] if k == "s" else c[k] for k in KEYS) for c in CASES + vgg7_wide(256) + vgg7_wide(2)}
    assert moved == 2 * len(wide) and len(wide) == len(CASES) + 9


def test_vgg_state_dict_layout():
    """cifar10_vggsmall after the module replacement: the reference's state_dict keys and shapes"""
    import torch

    import cim_quantization_amd._modules as my_nn
    from cim_quantization_amd.harness import models
    from cim_quantization_amd.harness.replace import ReplaceModuleTool
    with open(GOLDEN_VGG) as f:
        ref = json.load(f)
    torch.manual_seed(0)
    model = models.cifar10_vggsmall()
    assert isinstance(model, models.VGG) and tuple(model(torch.zeros(2, 3, 32, 32)).shape) == (2, 10)
    tool = ReplaceModuleTool(model, {"Conv2d": [my_nn.Conv2dLSQCiM]}, True, **ref["kwargs"])
    tool.replace()
    mine = [[k, list(v.shape), str(v.dtype)] for k, v in model.state_dict().items()]
    assert mine == ref["state"]
    assert [[c.nbits_w, c.nbits_a] for c in tool.convs] == ref["conv_bits"]  # first layer forced to w8a8
    convs = [m for m in model.modules() if isinstance(m, my_nn.Conv2dLSQCiM)]
    assert len(convs) == 6 and (convs[0].nbits_w, convs[0].nbits_a) == (8, 8)
    assert [cv.nbits_w for cv in convs[1:]] == [ref["kwargs"]["nbits_w"]] * 5
    assert any(k.startswith("features.3.") for k, _, _ in mine) and any(k == "classifier.weight" for k, _, _ in mine)
    assert [(cv.in_channels, cv.out_channels) for cv in convs] == [(3, 128), (128, 128), (128, 256), (256, 256),
                                                                    (256, 512), (512, 512)]


if __name__ == "__main__":
    path = sys.argv[1]
    lib_ = L.load()
    rows_ = [list(row) + answer(lib_, row) for row in descriptors()]
    with open(path, "w") as f_:
        f_.write('{"columns": %s,\n "rows": [\n' % json.dumps(COLUMNS))
        f_.write(",\n".join("  " + json.dumps(r) for r in rows_))
        f_.write("\n ]}\n")
    print(f"{len(rows_)} rows from {L.LIB_PATH}")
