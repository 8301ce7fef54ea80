"""CPU: the pooled store of the wide forward and the extended network calls as the host sees them (cimq_pool_abi,
cimq_module_pool_supported, cimq_module_forward_pool, cimq_net_ext, cimq_net_sizes_ex / cimq_net_forward_ex) -- the
availability symbol, the struct's layout, which layers pool, every refusal that needs no device (made-up addresses:
a refused call touches nothing), the pooled planes' sizes in a plan, and that no size or plan of the existing layers
moved."""
import ctypes
import json
import os
import subprocess

import pytest

from conftest import REPO
from pool_cases import CASES, FORMS, OFF_WIDE, P1, WIDE64, vgg7_pooled
from rect_cases import make_desc, route_names
from test_net_host import A, Plan
from wide_cases import case_id, wd

import cim_quantization_amd._lib as L
from cim_quantization_amd import build as cimq_build

INF = L.CIMQ_OPT_INFERENCE
MAX2 = L.CIMQ_POOL_MAX2


@pytest.fixture(scope="module")
def lib():
    cimq_build.build(verbose=False)
    return L.load()


def _ok(lib, d):
    ok = ctypes.c_int(-1)
    assert lib.cimq_module_pool_supported(ctypes.byref(d), ctypes.byref(ok)) == 0, lib.cimq_last_error()
    return ok.value


def test_availability(lib):
    assert lib.cimq_pool_abi() == 1 == L.pool_abi()
    assert L.CIMQ_POOL_MAX2 == 2 and L.NET_HEAD_FLATTEN == 1
    assert {"cimq_pool_abi", "cimq_module_pool_supported", "cimq_module_forward_pool", "cimq_net_sizes_ex",
            "cimq_net_forward_ex"} <= set(L.EXPORTED_SYMBOLS)
    # the other availability numbers are what they were
    assert (lib.cimq_abi_version(), lib.cimq_abi_minor()) == (16, 1)
    assert lib.cimq_w4a4_eval_abi() == 1 and lib.cimq_net_abi() == 1 and lib.cimq_wide_abi() == 1
    assert lib.cimq_shift_prepare_abi() == 1


def test_net_ext_layout_matches_header(tmp_path):
    """sizeof / offsetof of cimq_net_ext and the two constants from gcc on include/cimq.h equal the ctypes mirror"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cimq.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(cimq_net_ext));', '  printf("max2 %d\\n", CIMQ_POOL_MAX2);',
             '  printf("flatten %d\\n", CIMQ_NET_HEAD_FLATTEN);']
    for fname, _ in L.NetExt._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(cimq_net_ext, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in
               subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got.pop("size")) == ctypes.sizeof(L.NetExt) == 24
    assert int(got.pop("max2")) == L.CIMQ_POOL_MAX2 and int(got.pop("flatten")) == L.NET_HEAD_FLATTEN
    assert {k: int(v) for k, v in got.items()} == {f: getattr(L.NetExt, f).offset for f, _ in L.NetExt._fields_}


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_cases_pool(lib, c):
    d = make_desc(L, c, options=INF)
    assert route_names(L, d) == ("wide", "none", "none") and L.module_wide_plan(d)[0] == 1
    assert _ok(lib, d) == 1 and L.module_pool_supported(d) is True
    Wo = (c["W"] + 2 - 3) // c["s"][1] + 1
    assert Wo in (4, 8, 16, 32)


def test_cases_cover_the_kernel_forms():
    """the table holds each vertical-partner distance, each compile-time slice form and both K-step counts"""
    forms = []
    for c in CASES:
        cst = c["wb"] if (c["wb"] == c["ab"] and c["wbs"] == c["abs"] == 1 and 2 <= c["wb"] <= 4) else 0
        forms.append((-(-min(c["xbar"], c["C"] * 9) // 64), cst))
    assert forms == FORMS
    assert {f[1] for f in forms} == {0, 2, 3, 4} and {f[0] for f in forms} == {1, 2}
    assert {(c["W"] + 2 - 3) // c["s"][1] + 1 for c in CASES} == {4, 8, 16, 32}
    assert any(c["O"] % 64 for c in CASES) and any(c["O"] > 64 for c in CASES) and any(c["B"] % 2 for c in CASES)


@pytest.mark.parametrize("B", [256, 2])
def test_vgg7_pooled_layers(lib, B):
    cases = vgg7_pooled(B)
    assert [(c["C"], c["O"], c["H"]) for c in cases] == [(128, 128, 32), (256, 256, 16), (512, 512, 8)]
    for c in cases:
        assert _ok(lib, make_desc(L, c, options=INF)) == 1, case_id(c)


def test_not_poolable(lib):
    for c in CASES + vgg7_pooled(2):  # a training descriptor
        assert _ok(lib, make_desc(L, c)) == 0, case_id(c)
        assert _ok(lib, make_desc(L, c, options=L.CIMQ_OPT_RECOMPUTE)) == 0
    for c in OFF_WIDE:  # layers on the fwd5, v3, general and dense routes
        assert route_names(L, make_desc(L, c)) == c["route"], case_id(c)
        assert _ok(lib, make_desc(L, c, options=INF)) == 0, case_id(c)
    # a wide layer 64 columns wide
    d = make_desc(L, WIDE64, options=INF)
    assert route_names(L, d)[0] == "wide" and L.module_wide_plan(d)[0] == 1 and _ok(lib, d) == 0
    # the other ADC variants of a poolable shape run off the wide route
    for variant in (L.CIMQ_ADC_SHIFT_ROUND, L.CIMQ_ADC_STOCHASTIC):
        assert _ok(lib, make_desc(L, CASES[P1], variant=variant, options=INF)) == 0
    # null arguments
    assert lib.cimq_module_pool_supported(None, None) == L.CIMQ_EINVAL
    assert lib.cimq_module_pool_supported(ctypes.byref(d), None) == L.CIMQ_EINVAL


# ---- cimq_module_forward_pool with made-up device addresses ----
def _epi(residual=None, flags=0, reserved=0):
    e = L.Epilogue()
    e.scale, e.shift, e.residual, e.flags, e.reserved = A + 0x100, A + 0x200, residual, flags, reserved
    return e


def _call(lib, d, pool, epi=None, out=A + 0x10_0000, beta=None):
    epi = _epi() if epi is None else epi
    q = L.make_lsq_desc(-4, 3, 1e-3, 1e-3, 8)
    p = [A + 0x1000 * (i + 1) for i in range(7)]  # x, weight, alpha_act, alpha_weight, alpha_cim, bmask, signed
    rc = lib.cimq_module_forward_pool(ctypes.byref(d), ctypes.byref(q), p[0], p[1], p[2], p[3], p[4], beta, p[5], p[6],
                                      ctypes.byref(epi), pool, out, A + 0x40_0000, A + 0x80_0000, None)
    return rc, lib.cimq_last_error()


def test_forward_pool_refusals(lib):
    d = make_desc(L, CASES[P1], options=INF)
    for pool in (1, 3, -1, 4):
        rc, msg = _call(lib, d, pool)
        assert rc == L.CIMQ_EINVAL and b"pool must be" in msg, (pool, rc, msg)
    # every refusal of the epilogue call, with either pool value
    for pool in (0, MAX2):
        assert _call(lib, make_desc(L, CASES[P1]), pool)[0] == L.CIMQ_EINVAL            # a training descriptor
        for flags in (2, 3, 4):
            assert _call(lib, d, pool, _epi(flags=flags))[0] == L.CIMQ_EINVAL
        assert _call(lib, d, pool, _epi(reserved=1))[0] == L.CIMQ_EINVAL
        assert _call(lib, d, pool, _epi(residual=A + 0x20_0004))[0] == L.CIMQ_EINVAL     # misaligned
    # CIMQ_EUNSUPPORTED: off the wide route, 64 columns wide, beta_cim
    for c in OFF_WIDE:
        rc, msg = _call(lib, make_desc(L, c, options=INF), MAX2)
        assert rc == L.CIMQ_EUNSUPPORTED and b"off the wide route" in msg, (case_id(c), rc, msg)
    rc, msg = _call(lib, make_desc(L, WIDE64, options=INF), MAX2)
    assert rc == L.CIMQ_EUNSUPPORTED and b"wider than 32" in msg, (rc, msg)
    rc, msg = _call(lib, d, MAX2, beta=A + 0x9000)
    assert rc == L.CIMQ_EUNSUPPORTED and b"shift ADC" in msg, (rc, msg)


def test_forward_pool_overlap_uses_the_pooled_extent(lib):
    """out's extent is the pooled plane's, the residual's the unpooled one's"""
    c = CASES[P1]
    d = make_desc(L, c, options=INF)
    full = c["B"] * c["O"] * 16 * 16 * 4
    out = A + 0x10_0000
    for res in (out, out + full // 4 - 16, out - full + 16):
        rc, msg = _call(lib, d, MAX2, _epi(residual=res), out=out)
        assert rc == L.CIMQ_EINVAL and b"overlap" in msg, (hex(res), rc, msg)
    # a residual that starts where the pooled plane ends overlaps the unpooled out alone
    rc, msg = _call(lib, d, 0, _epi(residual=out + full // 4), out=out)
    assert rc == L.CIMQ_EINVAL and b"overlap" in msg


# ---- the network calls ----
def _wide_desc(C, O, H, B=2):
    return make_desc(L, wd(B, C, O, H, H), options=INF)


def _plan(descs, n_slots):
    p = Plan(names=("l1",) * len(descs), n_slots=n_slots)
    p.descs = list(descs)
    d0 = descs[0]
    p.shape = (d0.batch, d0.in_channels, d0.in_h, d0.in_w)
    return p


def _ext(pool=None, head_flags=0, reserved=(0, 0, 0)):
    e = L.make_net_ext(pool, head_flags)
    e.reserved[0], e.reserved[1], e.reserved[2] = reserved
    return e


def _sizes_ex(lib, p, ext):
    net = p.pack()
    n = max(p.n_slots, 1)
    fb, cb, ws = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)(), ctypes.c_size_t()
    rc = lib.cimq_net_sizes_ex(ctypes.byref(net), fb, cb, ctypes.byref(ws), None if ext is None else ctypes.byref(ext))
    return rc, list(fb), list(cb), ws.value


def _forward_ex(lib, p, ext):
    net = p.pack()
    n = max(p.n_slots, 1)
    sf, sc = (ctypes.c_void_p * n)(*p.sf[:n]), (ctypes.c_void_p * n)(*p.sc[:n])
    return lib.cimq_net_forward_ex(ctypes.byref(net), p.x, sf, sc, p.logits, p.ws, None,
                                   None if ext is None else ctypes.byref(ext))


def _both(lib, p, ext, code, word):
    """cimq_net_sizes_ex and cimq_net_forward_ex answer the same"""
    rc = _sizes_ex(lib, p, ext)[0]
    msg = lib.cimq_last_error()
    assert rc == code and word in msg, (rc, msg)
    rc = _forward_ex(lib, p, ext)
    msg = lib.cimq_last_error()
    assert rc == code and word in msg, (rc, msg)


def test_net_sizes_with_a_pooled_layer(lib):
    narrow, wide, after = _wide_desc(16, 128, 16), _wide_desc(128, 128, 16), _wide_desc(128, 32, 8)
    assert route_names(L, narrow)[0] != "wide" and route_names(L, wide)[0] == "wide"
    p = _plan([narrow, wide, after], 3)
    rc, fb, cb, ws = _sizes_ex(lib, p, _ext([0, MAX2, 0]))
    assert rc == 0, lib.cimq_last_error()
    assert fb == [2 * 128 * 16 * 16 * 4, 2 * 128 * 8 * 8 * 4, 2 * 32 * 8 * 8 * 4] and cb == [0, 0, 0]
    assert ws == max(L.query_sizes(d).fwd_workspace_bytes for d in p.descs)
    # a whole-tensor residual of the unpooled shape on the pooled layer
    p.layers[1].res_slot = 0
    assert _sizes_ex(lib, p, _ext([0, MAX2, 0]))[0] == 0, lib.cimq_last_error()
    # a consumer of the unpooled shape is refused
    q = _plan([narrow, wide, _wide_desc(128, 32, 16)], 3)
    _both(lib, q, _ext([0, MAX2, 0]), L.CIMQ_EINVAL, b"differs from its descriptor")
    # ... and without the pool it is the pooled-shape consumer that is
    _both(lib, p, _ext([0, 0, 0]), L.CIMQ_EINVAL, b"differs from its descriptor")
    _both(lib, p, None, L.CIMQ_EINVAL, b"differs from its descriptor")


def test_null_ext_is_the_old_call(lib):
    plans = [Plan(), Plan(names=("c48", "c48"), n_slots=2), Plan(names=(), n_slots=0)]
    plans[2].head.in_slot = -1
    bad = Plan()
    bad.layers[1].in_slot = 7
    for p in plans + [bad]:
        old = p.sizes(lib)
        old_msg = lib.cimq_last_error() if old[0] else b""
        new = _sizes_ex(lib, p, None)
        assert new == old and (not old[0] or lib.cimq_last_error() == old_msg)
        assert _sizes_ex(lib, p, _ext()) == old  # an all-zero ext adds nothing
    # (an accepted plan would launch on its made-up addresses: only the refused one goes through both forward calls)
    rc_old = bad.forward(lib)
    msg_old = lib.cimq_last_error()
    assert rc_old == L.CIMQ_EINVAL and _forward_ex(lib, bad, None) == rc_old and lib.cimq_last_error() == msg_old
    assert lib.cimq_net_sizes_ex(None, None, None, None, None) == L.CIMQ_EINVAL


def test_net_refusals(lib):
    narrow, wide, after = _wide_desc(16, 128, 16), _wide_desc(128, 128, 16), _wide_desc(128, 32, 8)
    mk = lambda: _plan([narrow, wide, after], 3)  # noqa: E731
    for v in (1, 3, -1):
        _both(lib, mk(), _ext([0, v, 0]), L.CIMQ_EINVAL, b"pool[1]")
    _both(lib, mk(), _ext([0, MAX2, 0], head_flags=2), L.CIMQ_EINVAL, b"head_flags")
    _both(lib, mk(), _ext([0, MAX2, 0], head_flags=3), L.CIMQ_EINVAL, b"head_flags")
    for k in range(3):
        r = [0, 0, 0]
        r[k] = 5
        _both(lib, mk(), _ext([0, MAX2, 0], reserved=r), L.CIMQ_EINVAL, b"reserved")
    # a pooled layer off the wide route
    _both(lib, _plan([narrow, _wide_desc(128, 128, 8)], 2), _ext([MAX2, 0]), L.CIMQ_EUNSUPPORTED, b"off the wide route")
    # a pooled wide layer 64 columns wide
    w64 = make_desc(L, WIDE64, options=INF)
    _both(lib, _plan([w64], 1), _ext([MAX2]), L.CIMQ_EUNSUPPORTED, b"wider than 32")
    # a pooled layer with a residual view (64 source channels into 128 from channel 32; the pooled layer reads x
    # itself): the wide route's own refusal, in the dry pass -- before any launch, on made-up addresses
    p = _plan([_wide_desc(128, 64, 16), wide], 2)
    p.layers[1].in_slot, p.layers[1].res_slot, p.layers[1].res_c0 = -1, 0, 32
    _both(lib, p, _ext([0, MAX2]), L.CIMQ_EUNSUPPORTED, b"the wide route reads no residual view")
    # ... and at stride 2: a 32 x 32 source over the 16 x 16 output of the pooled layer
    p = _plan([_wide_desc(128, 128, 32), make_desc(L, wd(2, 128, 128, 32, 32, s=2), options=INF), wide], 3)
    p.layers[2].res_slot, p.layers[2].res_stride = 0, 2
    _both(lib, p, _ext([0, 0, MAX2]), L.CIMQ_EUNSUPPORTED, b"layer 2: the wide route reads no residual view")
    # a pooled layer writing codes: the wide route's own refusal
    for mode in (2, 3):
        p = mk()
        p.layers[1].out_mode, p.layers[1].consumer, p.layers[2].in_codes = mode, 2, 1
        _both(lib, p, _ext([0, MAX2, 0]), L.CIMQ_EUNSUPPORTED, b"the wide route writes no out_codes")


def test_flatten_head_limit(lib):
    """C * H * W = 8192 (VGG7's 512 x 4 x 4) is accepted, 8196 is not"""
    last = _wide_desc(256, 512, 8)                     # pooled: [2, 512, 4, 4]
    p = _plan([last], 1)
    flat = _ext([MAX2], head_flags=L.NET_HEAD_FLATTEN)
    assert _sizes_ex(lib, p, flat)[0] == 0, lib.cimq_last_error()
    # a head-only plan over x itself: 2049 x 2 x 2 = 8196 features
    h = Plan(names=(), n_slots=0)
    h.head.in_slot = -1
    h.shape = (2, 2049, 2, 2)
    _both(lib, h, _ext(head_flags=L.NET_HEAD_FLATTEN), L.CIMQ_EUNSUPPORTED, b"8196 flattened features")
    h.shape = (2, 2048, 2, 2)
    assert _sizes_ex(lib, h, _ext(head_flags=L.NET_HEAD_FLATTEN))[0] == 0, lib.cimq_last_error()
    # without the flag the head pools: 2049 channels pass, and the unpooled 512 x 8 x 8 map flattened does not
    assert _sizes_ex(lib, h, _ext())[0] == 0
    _both(lib, p, _ext([0], head_flags=L.NET_HEAD_FLATTEN), L.CIMQ_EUNSUPPORTED, b"flattened features")


def test_python_side_refusals():
    """forward_fused's pool keyword: anything but None / 2, and codes with it, raise before a device is touched"""
    import torch

    import cim_quantization_amd._modules as my_nn
    m = my_nn.Conv2dLSQCiM(128, 32, 3, 1, 1, bias=False, nbits_w=3, nbits_a=3, nbits_alpha=8, wbitslice=1, abitslice=1,
                           xbar=128, adcbits=1.5, stochastic_quant=False)
    x = torch.zeros(2, 128, 16, 16)
    sc = torch.ones(32)
    with torch.no_grad():
        with pytest.raises(ValueError, match="pool must be"):
            m.forward_fused(x, sc, sc, pool=3)
        with pytest.raises(ValueError, match="no out_quant"):
            m.forward_fused(x, sc, sc, pool=2, out_quant=m)
        assert m.pool_ready(x) is False  # CPU tensors: off the library path
        with pytest.raises(RuntimeError, match="pool_ready"):
            m.forward_fused(x, sc, sc, pool=2)
    from cim_quantization_amd.harness.fuse import FusedEval, _is_pool2, _vgg_triples
    from cim_quantization_amd.harness.models import VGG
    import torch.nn as nn
    assert _is_pool2(nn.MaxPool2d(2, 2)) and _is_pool2(nn.MaxPool2d((2, 2)))
    assert not _is_pool2(nn.MaxPool2d(3, 2)) and not _is_pool2(nn.MaxPool2d(2, 2, ceil_mode=True))
    assert not _is_pool2(nn.MaxPool2d(2, 1)) and not _is_pool2(nn.MaxPool2d(2, 2, padding=1))
    assert not _is_pool2(nn.AvgPool2d(2, 2))
    v = VGG(plan=(16, 16, "M", 32, 32, "M"))
    assert [(k, p) for k, _, _, p in _vgg_triples(v)] == [(0, False), (3, True), (7, False), (10, True)]
    f = FusedEval(v, pool=True)
    assert f.pool is True and f.pooled == [] and FusedEval(v).pool is False


# ---- nothing that existed moved ----
PLANS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pool_parent_plans.json")


def _plan_rows(lib):
    """[ok, chunks, groups, tiles] of cimq_module_wide_plan for every descriptor row of wide_parent_table.json"""
    import test_wide_routes_host as W
    with open(W.TABLE) as f:
        rows = json.load(f)["rows"]
    out = []
    for r in rows:
        d = W.row_desc(r)
        f4 = (ctypes.c_int * 4)()
        rc = lib.cimq_module_wide_plan(ctypes.byref(d), f4)
        out.append([rc] + list(f4))
    return rows, out


def test_parent_sizes_and_plans_unchanged(lib):
    """every row of tests/golden/wide_parent_table.json: cimq_query_sizes answers what the table holds, and
    cimq_module_wide_plan what the parent commit's library (785ea02) answered -- tests/golden/pool_parent_plans.json,
    recorded with ``CIMQ_LIB_PATH=<the parent's libcimq.so> python tools/record_wide_plans.py <path>`` -- also after a
    pool query of the same descriptor"""
    import test_wide_routes_host as W
    with open(PLANS) as f:
        want = json.load(f)["plans"]
    rows, got = _plan_rows(lib)
    assert len(want) == len(rows) and got == want
    assert sum(p[1] for p in want) >= 2 * (len(W.CASES) + 9)  # the wide rows are there
    for r in rows:
        d = W.row_desc(r)
        ok = ctypes.c_int()
        lib.cimq_module_pool_supported(ctypes.byref(d), ctypes.byref(ok))
        assert W.answer(lib, r)[4:] == r[W.NDESC + 4:W.NDESC + 9], r[:W.NDESC]
    assert _plan_rows(lib)[1] == want

