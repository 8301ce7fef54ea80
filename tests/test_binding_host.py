"""CPU: the descriptors the Python binding builds (functional.module_descs and the primitive behind the training
shift form) against the bytes recorded before the binding got its one marshalling path
(tests/golden/binding_descs.json, written by tests/golden/make_binding_descs.py), and the size equality that lets
every module entry point allocate its ctx with module_ctx_bytes.  Host queries only: no device work."""
import json
import os

import pytest

import cim_quantization_amd._lib as L
import cim_quantization_amd._modules as my_nn
from cim_quantization_amd import build as cimq_build
from cim_quantization_amd import functional as F

with open(os.path.join(os.path.dirname(__file__), "golden", "binding_descs.json")) as f:
    CASES = json.load(f)
IDS = [f"{c['name']}-{'inference' if c['inference'] else 'training'}" for c in CASES]


def _descs(c):
    ctor = dict(c["ctor"])
    for k in ("kernel_size", "stride", "padding"):
        if isinstance(ctor[k], list):
            ctor[k] = tuple(ctor[k])
    m = my_nn.Conv2dLSQCiM(bias=False, **ctor)
    for a, v in c["attrs"].items():
        setattr(m, a, v)
    assert (m.alpha_cim is None) == c["alpha_cim_is_none"]
    shape = tuple(c["shape"])
    if c["how"] == "shift_primitive":
        return F._shift_module_descs(shape, m.weight, m.stride, m.padding, m.dilation, m.nbits_a, m.abitslice,
                                     m.nbits_w, m.wbitslice, m.xbar, m.nbits_alpha)
    return F.module_descs(m, shape, c["inference"])


def test_the_table_covers_the_binding():
    names = {c["name"] for c in CASES}
    assert names == {"w3a3", "w3a3_recompute", "w8a8_first", "w4a4_bs1", "w4a4_bs2", "stride2", "k1x1", "adc4",
                     "xbar64", "rect_1x3", "shift_w2a2"}
    assert any(c["how"] == "shift_primitive" and not c["inference"] for c in CASES)
    assert [c["alpha_cim_is_none"] for c in CASES if c["name"] == "adc4"] == [True, True]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_descriptors_are_the_recorded_ones(c):
    desc, lsq = _descs(c)
    assert bytes(desc).hex() == c["desc"]
    for k in ("qn_w", "qp_w", "gscale_a", "gscale_w", "nbits_alpha", "flags"):
        assert getattr(lsq, k) == c[k], k
    assert not lsq.wprep


def test_a_training_shift_layer_has_descriptors_but_no_prepared_side():
    """module_descs answers for a shift-ADC layer in training too (its forward builds that pair); only the
    prepared weight side is refused there, as before."""
    c = next(c for c in CASES if c["how"] == "shift_primitive")
    ctor = dict(c["ctor"])
    m = my_nn.Conv2dLSQCiM(bias=False, **ctor)
    desc, _ = F.module_descs(m, tuple(c["shape"]))
    assert bytes(desc).hex() == c["desc"]
    with pytest.raises(ValueError, match="forward-only"):
        F._prepare_item(m, tuple(c["shape"]))


@pytest.mark.parametrize("c", [c for c in CASES if c["inference"] or c["how"] == "shift_primitive"],
                         ids=[i for i, c in zip(IDS, CASES) if c["inference"] or c["how"] == "shift_primitive"])
def test_module_ctx_is_the_whole_ctx_where_ctx_bytes_was_used(c):
    """_layer_call sizes every module entry point's ctx with module_ctx_bytes.  The shift forward, the epilogue /
    codes calls and the one-call plan used ctx_bytes before: allowed because the two are equal for the training
    shift descriptor and for every forward-only descriptor."""
    cimq_build.build(verbose=False)
    sizes = L.query_sizes(_descs(c)[0])
    assert sizes.ctx_bytes == sizes.module_ctx_bytes > 0


def test_grads_places_by_name():
    names = F._CimModuleConv._ARGS
    assert names[:5] == ("x", "weight", "alpha_act", "alpha_weight", "alpha_cim") and len(names) == 22
    g = F._grads(names, x=1, alpha_cim=5)
    assert g == (1, None, None, None, 5) + (None,) * 17
    assert F.get_cim_output_signed._ARGS.index("alpha_cim") == 12 and len(F.get_cim_output_signed._ARGS) == 17
    with pytest.raises(ValueError):
        F._grads(names, no_such_argument=1)
