"""CPU: the ideal-ADC conv's large-layer backward (CIMQ_OPT_WIDE_BWD on cimq_ideal_desc, cimq_ideal_wide_*) on the
cross-compiled library -- availability, arities, the plan on and off its shape class.  Host logic only."""
import pytest

import cim_quantization_amd._lib as L
from cim_quantization_amd import build as cimq_build
from test_abi_host import header_arities
from test_ideal_host import desc

HINT = L.CIMQ_OPT_WIDE_BWD
VGG_SMALL = [(128, 128, 32), (128, 256, 16), (256, 256, 16), (256, 512, 8), (512, 512, 8)]  # (C, O, H = W)


@pytest.fixture(scope="module")
def lib():
    cimq_build.build(verbose=False)
    return L.load()


def test_abi_and_arities(lib):
    assert lib.cimq_ideal_wide_abi() == 1
    ar = header_arities()
    for sym in ("cimq_ideal_wide_abi", "cimq_ideal_wide_plan"):
        assert sym in L.EXPORTED_SYMBOLS
        assert len(getattr(lib, sym).argtypes) == ar[sym], sym


@pytest.mark.parametrize("c,o,h", VGG_SMALL)
def test_vgg_small_trains_under_the_hint(lib, c, o, h):
    kw = dict(B=256, C=c, O=o, H=h, W=h)
    assert L.ideal_plan(desc(options=HINT, **kw))[0] == 1
    wide = L.ideal_wide_plan(desc(options=HINT, **kw))
    assert wide[0] == 1 and 0 < wide[5] <= 160 * 1024 - 512
    assert L.ideal_plan(desc(**kw))[0] == 0 and "vendor" in lib.cimq_last_error().decode()
    assert L.ideal_wide_plan(desc(**kw))[0] == 0


def test_plan_counts_of_the_gpu_cases():
    """(ok, grad_x workgroups per image, output chunks, stages per slab, slabs, LDS bytes)"""
    w4 = L.ideal_wide_plan(desc(B=2, C=128, O=256, H=2, W=32, bits=2, options=HINT))
    assert w4[0] == 1 and w4[2] >= 2
    w6 = L.ideal_wide_plan(desc(B=5, C=128, O=32, H=16, W=16, options=HINT))
    assert w6[0] == 1 and w6[3] >= 2 and w6[4] >= 2


@pytest.mark.parametrize("kw", [
    dict(s=2, H=16, W=16), dict(C=64), dict(k=5, p=2), dict(H=8, W=64), dict(C=3), dict(options=L.CIMQ_OPT_INFERENCE),
], ids=["stride2", "C64", "5x5", "W64", "C3", "inference"])
def test_off_the_plan_the_hint_changes_nothing(lib, kw):
    kw = dict(dict(B=2, C=128, O=32, H=8, W=8), **kw)
    plain = desc(**kw)
    kw["options"] = kw.get("options", 0) | HINT
    hinted = desc(**kw)
    assert L.ideal_plan(plain)[0] == 1
    assert L.ideal_plan(hinted) == L.ideal_plan(plain)
    assert L.ideal_sizes(hinted) == L.ideal_sizes(plain)
    assert L.ideal_wide_plan(hinted)[0] == 0
    assert lib.cimq_last_error().decode().startswith("ideal wide:")
