"""CPU: the ideal-ADC conv's C ABI (cimq_ideal_*) on the cross-compiled library -- availability, the header's
arities, the plan counts tests/test_gpu_ideal.py's cases rely on, and the refusals.  Host logic only."""
import ctypes

import pytest

import cim_quantization_amd._lib as L
from cim_quantization_amd import build as cimq_build
from test_abi_host import header_arities

NEW = ("cimq_ideal_abi", "cimq_ideal_plan", "cimq_ideal_sizes", "cimq_ideal_forward", "cimq_ideal_backward")


@pytest.fixture(scope="module")
def lib():
    cimq_build.build(verbose=False)
    return L.load()


def desc(B=2, C=16, O=16, H=8, W=8, k=3, s=1, p=1, bits=3, **kw):
    kw.setdefault("bits_w", bits)
    kw.setdefault("bits_a", bits)
    return L.make_ideal_desc(B, C, H, W, O, kw.pop("KH", k), kw.pop("KW", k), (s, s), (p, p), **kw)


def test_abi_and_arities(lib):
    assert lib.cimq_ideal_abi() == 1
    ar = header_arities()
    for sym in NEW:
        assert sym in L.EXPORTED_SYMBOLS
        assert len(getattr(lib, sym).argtypes) == ar[sym], sym


def test_plan_counts_of_the_gpu_cases():
    """(ok, m-tiles per image, patch chunks, grad_x bands per image, grad_w slabs)"""
    assert L.ideal_plan(desc())[:3] == (1, 1, 1)
    assert L.ideal_plan(desc(C=144, bits=4))[2] == 1               # I7 as the issue states it: one chunk ...
    assert L.ideal_plan(desc(C=1032, bits=4))[2] >= 2              # ... I7c: raised until the patch is chunked
    ok, mt, _, bands, slabs = L.ideal_plan(desc(B=5, H=16, W=16))  # I8
    assert ok == 1 and mt >= 2 and bands >= 2 and slabs >= 2


@pytest.mark.parametrize("kw,code,word", [
    (dict(bits_a=9), L.CIMQ_EUNSUPPORTED, "bits"),
    (dict(KH=8), L.CIMQ_EUNSUPPORTED, "kernel"),
    (dict(s=3), L.CIMQ_EUNSUPPORTED, "stride"),
    (dict(C=8192), L.CIMQ_EUNSUPPORTED, "65536"),
    (dict(reserved=1), L.CIMQ_EINVAL, "reserved"),
    (dict(options=8), L.CIMQ_EINVAL, "option"),
    (dict(B=0), L.CIMQ_EINVAL, "geometry"),
])
def test_refusals(lib, kw, code, word):
    out = (ctypes.c_int * 5)()
    d = desc(**kw)
    assert lib.cimq_ideal_plan(ctypes.byref(d), out) == code
    assert word in lib.cimq_last_error().decode()
    assert out[0] == 0
    assert lib.cimq_ideal_sizes(ctypes.byref(d), None, None) == code
    # the launching calls validate the descriptor before anything else: no device work on a refusal
    assert lib.cimq_ideal_forward(ctypes.byref(d), *([None] * 8)) == code


def test_no_field_for_dilation_or_groups():
    names = {f for f, _ in L.IdealDesc._fields_}
    assert not names & {"dilation_h", "dilation_w", "groups"}


def test_null_pointers_and_inference_backward(lib):
    d, di = desc(), desc(options=L.CIMQ_OPT_INFERENCE)
    assert lib.cimq_ideal_plan(None, (ctypes.c_int * 5)()) == L.CIMQ_EINVAL
    assert lib.cimq_ideal_plan(ctypes.byref(d), None) == L.CIMQ_EINVAL
    assert lib.cimq_ideal_forward(ctypes.byref(d), *([None] * 8)) == L.CIMQ_EINVAL
    assert "null" in lib.cimq_last_error().decode()
    assert lib.cimq_ideal_backward(ctypes.byref(d), *([None] * 12)) == L.CIMQ_EINVAL
    assert lib.cimq_ideal_backward(ctypes.byref(di), *([None] * 12)) == L.CIMQ_EINVAL
    assert "inference" in lib.cimq_last_error().decode()


def test_large_layers_train_on_the_vendor_conv(lib):
    """the measured gate: above 2^30 padded MACs only the forward-only descriptor is taken"""
    kw = dict(B=256, C=128, O=128, H=32, W=32)
    d, di = desc(**kw), desc(options=L.CIMQ_OPT_INFERENCE, **kw)
    assert L.ideal_plan(d)[0] == 0 and "vendor" in lib.cimq_last_error().decode()
    assert L.ideal_plan(di)[0] == 1
    assert L.ideal_plan(desc(B=256, C=64, O=64))[0] == 1  # ResNet-20's heaviest shape trains in the library


def test_sizes():
    d, di = desc(), desc(options=L.CIMQ_OPT_INFERENCE)
    ctx, ws = L.ideal_sizes(d)
    ctx_i, ws_i = L.ideal_sizes(di)
    assert ctx > 0 and ws > 0
    assert ws_i == ws
    assert 0 < ctx_i < ctx  # documented: an inference ctx holds the forward's fragments alone
    assert L.ideal_plan(di) == L.ideal_plan(d)
