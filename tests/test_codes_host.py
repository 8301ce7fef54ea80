"""CPU: activation codes between convs (ABI 16, minor 1) as the host sees them -- the ABI constants, the layout of
cimq_act_codes, every refusal of cimq_module_forward_codes (host checks, made before any device work), what
cimq_module_codes_supported answers for every test case and ResNet-20 layer, the unchanged buffer sizes, and the
torch twin of the code definition."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import REPO
from test_abi_host import header_symbols
from test_inference_host import CASES, INF, all_descs, case_desc

import cim_quantization_amd._lib as L
from cim_quantization_amd import build as cimq_build


@pytest.fixture(scope="module")
def lib():
    cimq_build.build(verbose=False)
    return L.load()


def test_abi_version_and_minor(lib):
    assert lib.cimq_abi_version() == 16 == L.ABI_VERSION
    assert lib.cimq_abi_minor() == 1 == L.ABI_MINOR
    with open(os.path.join(REPO, "include", "cimq.h")) as f:
        txt = f.read()
    assert int(re.search(r"#define\s+CIMQ_ABI_VERSION\s+(\d+)", txt).group(1)) == 16
    assert int(re.search(r"#define\s+CIMQ_ABI_MINOR\s+(\d+)", txt).group(1)) == 1
    assert L.CIMQ_CODES_NO_FLOAT == 1


def test_header_binding_and_library_agree(lib):
    new = {"cimq_abi_minor", "cimq_module_forward_codes", "cimq_module_codes_supported"}
    assert new <= set(L.EXPORTED_SYMBOLS)
    assert header_symbols() == sorted(L.EXPORTED_SYMBOLS)
    raw = ctypes.CDLL(L.LIB_PATH)
    for sym in L.EXPORTED_SYMBOLS:
        assert hasattr(raw, sym), sym


def test_act_codes_layout_matches_header(tmp_path):
    """sizeof / offsetof of cimq_act_codes from gcc on include/cimq.h equal the ctypes mirror, field by field in
    the issue's order"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cimq.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(cimq_act_codes));', '  printf("nofloat %d\\n", CIMQ_CODES_NO_FLOAT);',
             '  printf("minor %d\\n", CIMQ_ABI_MINOR);']
    for fname, _ in L.ActCodes._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(cimq_act_codes, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in
               subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines() if line)
    assert int(got.pop("size")) == ctypes.sizeof(L.ActCodes) == 40
    assert int(got.pop("nofloat")) == L.CIMQ_CODES_NO_FLOAT
    assert int(got.pop("minor")) == L.ABI_MINOR
    assert [f for f, _ in L.ActCodes._fields_] == ["x_codes", "out_codes", "out_alpha_act", "out_gscale_a", "out_qp",
                                                   "flags", "reserved"]
    for fname, v in got.items():
        assert int(v) == getattr(L.ActCodes, fname).offset, fname


# made-up device addresses: every refusal below is decided on the host before anything is dereferenced or
# launched
A = 0x7000_0000_0000
X, XQ, OUT, OQ, RES = A + 0x100_0000, A + 0x200_0000, A + 0x300_0000, A + 0x400_0000, A + 0x500_0000


def _epi(scale=A + 0x100, shift=A + 0x200, residual=None, flags=0, reserved=0):
    e = L.Epilogue()
    e.scale, e.shift, e.residual, e.flags, e.reserved = scale, shift, residual, flags, reserved
    return e


def _io(x_codes=None, out_codes=OQ, alpha=A + 0x300, gs=1e-3, qp=7.0, flags=0, reserved=0):
    io = L.ActCodes()
    io.x_codes, io.out_codes, io.out_alpha_act = x_codes, out_codes, alpha
    io.out_gscale_a, io.out_qp, io.flags, io.reserved = gs, qp, flags, reserved
    return io


def _call(lib, d, io, epi="default", x=X, out=OUT, beta=None):
    if epi == "default":
        epi = _epi()
    q = L.make_lsq_desc(-4, 3, 1e-3, 1e-3, 8)
    p = [A + 0x1000 * (i + 1) for i in range(6)]  # weight, alpha_act, alpha_weight, alpha_cim, bmask, signed
    return lib.cimq_module_forward_codes(ctypes.byref(d), ctypes.byref(q), None if io is None else ctypes.byref(io), x,
                                         p[0], p[1], p[2], p[3], beta, p[4], p[5],
                                         None if epi is None else ctypes.byref(epi), out, A + 0x40_0000, A + 0x80_0000,
                                         None)


def _refused(lib, rc, word, code=L.CIMQ_EINVAL):
    assert rc == code, (rc, lib.cimq_last_error())
    msg = lib.cimq_last_error()
    assert msg and b"cimq_module_forward_codes" in msg and word in msg, msg


def test_refuses_training_descriptor(lib):
    _refused(lib, _call(lib, case_desc("l1", 0), _io()), b"CIMQ_OPT_INFERENCE")
    _refused(lib, _call(lib, case_desc("l1", L.CIMQ_OPT_RECOMPUTE), _io()), b"CIMQ_OPT_INFERENCE")


def test_refuses_null_io_and_epilogue(lib):
    d = case_desc("l1", INF)
    _refused(lib, _call(lib, d, None), b"null io")
    _refused(lib, _call(lib, d, _io(), epi=None), b"null epilogue")
    _refused(lib, _call(lib, d, _io(), epi=_epi(scale=None)), b"null epilogue")


def test_refuses_reserved_and_unknown_flags(lib):
    d = case_desc("l1", INF)
    _refused(lib, _call(lib, d, _io(reserved=1)), b"reserved")
    _refused(lib, _call(lib, d, _io(reserved=-3)), b"reserved")
    for flags in (2, 4, 3, -1, 1 << 30):
        _refused(lib, _call(lib, d, _io(flags=flags)), b"unknown flags")


def test_refuses_no_float_without_out_codes(lib):
    d = case_desc("l1", INF)
    _refused(lib, _call(lib, d, _io(out_codes=None, flags=L.CIMQ_CODES_NO_FLOAT)), b"CIMQ_CODES_NO_FLOAT")
    _refused(lib, _call(lib, d, _io(x_codes=XQ, out_codes=None, flags=L.CIMQ_CODES_NO_FLOAT)), b"CIMQ_CODES_NO_FLOAT")


def test_refuses_bad_consumer(lib):
    d = case_desc("l1", INF)
    _refused(lib, _call(lib, d, _io(alpha=None)), b"out_alpha_act")
    for qp in (0.0, 0.5, 3.5, 255.0, 256.0, -1.0, float("nan"), float("inf")):
        _refused(lib, _call(lib, d, _io(qp=qp)), b"out_qp")


def test_refuses_misaligned_code_buffers(lib):
    d = case_desc("l1", INF)
    for off in (1, 4, 8, 12):
        _refused(lib, _call(lib, d, _io(out_codes=OQ + off)), b"aligned")
        _refused(lib, _call(lib, d, _io(x_codes=XQ + off)), b"aligned")


@pytest.mark.parametrize("name", ["l1", "l2s2", "c48"])
def test_refuses_out_codes_overlapping(lib, name):
    d = case_desc(name, INF)
    Ho = (d.in_h + 2 * d.pad_h - d.kernel_h) // d.stride_h + 1
    n_out = d.batch * d.out_channels * Ho * Ho          # bytes of out_codes; out and the residual are 4 n_out
    n_in = d.batch * d.in_channels * d.in_h * d.in_w    # bytes of x_codes; x is 4 n_in
    for oq in (OUT, OUT + 4 * n_out - 16, OUT - n_out + 16):
        _refused(lib, _call(lib, d, _io(out_codes=oq)), b"overlaps out")
    for oq in (XQ, XQ + n_in - 16, XQ - n_out + 16):
        _refused(lib, _call(lib, d, _io(x_codes=XQ, out_codes=oq)), b"overlaps x_codes")
    for oq in (X, X + 4 * n_in - 16, X - n_out + 16):
        _refused(lib, _call(lib, d, _io(out_codes=oq)), b"overlaps x")
    for oq in (RES, RES + 4 * n_out - 16, RES - n_out + 16):
        _refused(lib, _call(lib, d, _io(out_codes=oq), epi=_epi(residual=RES)), b"overlaps the residual")


def test_unsupported_answers(lib):
    # a layer whose Qp does not fit a byte with the NaN code reads no codes
    _refused(lib, _call(lib, case_desc("conv1", INF), _io(x_codes=XQ, out_codes=None)), b"lsq_qp", L.CIMQ_EUNSUPPORTED)
    _refused(lib, _call(lib, case_desc("l1", INF, lsq_qp=255.0), _io(x_codes=XQ, out_codes=None)), b"lsq_qp",
             L.CIMQ_EUNSUPPORTED)
    # the dense kernels write none
    _refused(lib, _call(lib, case_desc("dense", INF), _io()), b"dense", L.CIMQ_EUNSUPPORTED)


def _supported(lib, d):
    a, b = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.cimq_module_codes_supported(ctypes.byref(d), ctypes.byref(a), ctypes.byref(b)) == 0, lib.cimq_last_error()
    return a.value, b.value


def test_codes_supported(lib):
    """in_ok is 1 except for the w8a8 first conv (Qp = 255: the NaN code would not fit a byte); out_ok is 1 on the
    fwd5, v3 and general forward routes and 0 on the dense one"""
    seen = set()
    for name, d in all_descs(INF):
        in_ok, out_ok = _supported(lib, d)
        route = L.ROUTE_NAMES[L.module_route(d)[0]]
        seen.add(route)
        assert in_ok == (0 if name == "conv1" else 1), name
        assert out_ok == (1 if route in ("fwd5", "v3", "general") else 0), (name, route)
        if name in CASES:
            assert route == CASES[name][-1]
        # the answer is for the forward-only form whatever the option bits say; either pointer may be NULL
        d0 = case_desc(name, 0) if name in CASES else d
        assert _supported(lib, d0) == (in_ok, out_ok)
        a = ctypes.c_int(-1)
        assert lib.cimq_module_codes_supported(ctypes.byref(d), ctypes.byref(a), None) == 0 and a.value == in_ok
        assert lib.cimq_module_codes_supported(ctypes.byref(d), None, ctypes.byref(a)) == 0 and a.value == out_ok
    assert seen == {"fwd5", "v3", "general", "dense"}
    assert lib.cimq_module_codes_supported(None, None, None) == L.CIMQ_EINVAL
    assert L.codes_supported(case_desc("l1", INF)) == (True, True)
    assert L.codes_supported(case_desc("dense", INF)) == (True, False)


# cimq_query_sizes of every case and ResNet-20 layer at B = 256, forward-only form, as the parent commit reports
# them: (ctx_bytes, fwd_workspace_bytes, wprep_bytes).  The feature needs no extra workspace.
def test_query_sizes_unchanged(lib):
    import json
    with open(os.path.join(REPO, "tests", "golden", "codes_sizes.json")) as f:
        want = json.load(f)
    got = {}
    for opt in (0, INF):
        for name, d in all_descs(opt):
            s = L.query_sizes(d)
            got[f"{name}/{opt}"] = [s.ctx_bytes, s.fwd_workspace_bytes, s.bwd_workspace_bytes, s.wprep_bytes,
                                    s.module_ctx_bytes]
    assert got == want


# ---------------------------------------------------------------------------------------------------
# the torch twin
# ---------------------------------------------------------------------------------------------------
def test_act_codes_twin():
    """Conv2dLSQCiM.act_codes: rint(clamp(y / sa, 0, Qp)) with ties to even, Qp + 1 for NaN, sa the fp32
    grad_scale value of alpha_act (a power of two gives sa == alpha_act exactly)"""
    import cim_quantization_amd._modules as my_nn
    from cim_quantization_amd import functional as F
    m = my_nn.Conv2dLSQCiM(16, 16, 3, 1, 1, bias=False, nbits_w=3, nbits_a=3, nbits_alpha=8, wbitslice=1, abitslice=1,
                           xbar=128, adcbits=1.5, signed_xbar=True, stochastic_quant=False)
    with torch.no_grad():
        m.alpha_act.fill_(0.25)
    y = torch.tensor([-1.0, 0.0, 0.124, 0.125, 0.126, 0.375, 0.625, 1.7, 1.75, 1.8, 100.0, float("inf"),
                      float("-inf"), float("nan")]).view(1, 1, 1, -1)
    alpha, gs, qp = m._code_quant(y.numel())
    assert qp == 7.0 and float(F.act_code_step(alpha, gs)) == 0.25
    got = m.act_codes(y).view(-1).tolist()
    assert got == [0, 0, 0, 0, 1, 2, 2, 7, 7, 7, 7, 7, 0, 8]
    assert m.act_codes(y).dtype == torch.uint8


def test_python_entry_refuses_differentiable_call():
    from cim_quantization_amd import functional as F
    w = torch.zeros(16, 16, 3, 3, requires_grad=True)
    x = torch.zeros(1, 16, 8, 8, dtype=torch.uint8)
    one = torch.ones(1)
    with pytest.raises(RuntimeError, match="forward only"):
        F.cim_module_conv_codes(x, w, one, one, None, torch.ones(1, 1, 3, 3, 1, 1), one, 1, 1, 1, 3, 1, 3, 1, 6,
                                128, 8, torch.ones(16), torch.zeros(16))


def test_fused_eval_codes_wiring_cpu():
    """on a plain (unreplaced) resnet20 no conv handles codes: every edge stays fp32 and the logits are those of
    FusedEval(model)"""
    from cim_quantization_amd.harness import models
    from cim_quantization_amd.harness.fuse import FusedEval
    from test_epilogue_host import randomise_bn
    torch.manual_seed(11)
    model = models.resnet20().eval()
    randomise_bn(model, 12)
    x = torch.randn(2, 3, 32, 32)
    with torch.no_grad():
        fused = FusedEval(model, codes=True)
        assert torch.equal(fused(x), FusedEval(model)(x))
        assert fused.code_edges == []
