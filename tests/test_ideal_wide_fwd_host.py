"""CPU: the ideal-ADC conv's large-layer forward (CIMQ_OPT_WIDE_BWD on cimq_ideal_desc, cimq_ideal_wide_fwd_*) on the
cross-compiled library -- availability, arities, the plan on and off its shape class.  Host logic only."""
import pytest

import cim_quantization_amd._lib as L
from cim_quantization_amd import build as cimq_build
from test_abi_host import header_arities
from test_ideal_host import desc
from test_ideal_wide_host import VGG_SMALL

HINT = L.CIMQ_OPT_WIDE_BWD


@pytest.fixture(scope="module")
def lib():
    cimq_build.build(verbose=False)
    return L.load()


def test_abi_and_arities(lib):
    assert lib.cimq_ideal_wide_fwd_abi() == 1
    ar = header_arities()
    for sym in ("cimq_ideal_wide_fwd_abi", "cimq_ideal_wide_fwd_plan"):
        assert sym in L.EXPORTED_SYMBOLS
        assert len(getattr(lib, sym).argtypes) == ar[sym], sym


@pytest.mark.parametrize("inference", [0, L.CIMQ_OPT_INFERENCE], ids=["training", "inference"])
@pytest.mark.parametrize("c,o,h", VGG_SMALL)
def test_vgg_small_is_on_the_plan(lib, c, o, h, inference):
    ok, mt, nch, gpw, ny, lds = L.ideal_wide_fwd_plan(desc(B=256, C=c, O=o, H=h, W=h, options=HINT | inference))
    assert ok == 1 and mt == h * h // 64 and nch == 1  # one chunk: the patch is staged once per workgroup
    assert gpw >= 1 and ny >= 1 and 0 < lds <= 160 * 1024 - 512


@pytest.mark.parametrize("kw", [
    dict(options=0), dict(bits_a=8), dict(s=2, H=16, W=16), dict(C=64), dict(k=5, p=2), dict(H=8, W=64), dict(C=3),
], ids=["no-hint", "a8", "stride2", "C64", "5x5", "W64", "C3"])
def test_off_the_plan_the_hint_changes_nothing(lib, kw):
    kw = dict(dict(B=2, C=128, O=32, H=8, W=8, options=HINT), **kw)
    for inference in (0, L.CIMQ_OPT_INFERENCE):
        hinted = desc(**dict(kw, options=kw["options"] | inference))
        plain = desc(**dict(kw, options=inference))
        assert L.ideal_wide_fwd_plan(hinted)[0] == 0
        assert lib.cimq_last_error().decode().startswith("ideal wide fwd:")
        assert L.ideal_plan(plain)[0] == 1
        if kw.get("bits_a") == 8 and not inference:
            continue  # (a training a8 descriptor of this class is on the backward pair's plan, which the hint moves)
        assert L.ideal_plan(hinted) == L.ideal_plan(plain)
        assert L.ideal_sizes(hinted) == L.ideal_sizes(plain)


def test_plan_counts_of_the_gpu_cases():
    """(ok, tiles per image, channel chunks, output groups per workgroup, workgroups in blockIdx.y, LDS bytes)"""
    f4 = L.ideal_wide_fwd_plan(desc(B=2, C=128, O=320, H=2, W=32, bits=2, options=HINT))
    assert f4[0] == 1 and f4[3] > 1  # the resident-patch loop
    f5 = L.ideal_wide_fwd_plan(desc(B=1, C=640, O=32, H=2, W=32, options=HINT))
    assert f5[:3] == (1, 1, 2)  # two channel chunks (ncx = 320)
    assert L.ideal_plan(desc(B=1, C=640, O=32, H=2, W=32, options=HINT))[2] == 2  # ... as ideal_plan cuts them
