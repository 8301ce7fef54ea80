"""CPU: the output epilogue (ABI 16) as the host sees it -- the ABI constant, the layout of cimq_epilogue,
every refusal of cimq_module_forward_epilogue (host checks, made before any device work), BatchNorm folding
against the fp64 formula, and the wiring of harness.fuse.FusedEval on a plain (unreplaced) resnet20."""
import ctypes
import os
import subprocess

import pytest
import torch

from conftest import REPO
from test_inference_host import INF, case_desc

import cim_quantization_amd._lib as L
from cim_quantization_amd import build as cimq_build


@pytest.fixture(scope="module")
def lib():
    cimq_build.build(verbose=False)
    return L.load()


def test_abi_version(lib):
    assert lib.cimq_abi_version() == 16 == L.ABI_VERSION
    assert L.CIMQ_EPI_RELU == 1
    assert "cimq_module_forward_epilogue" in L.EXPORTED_SYMBOLS


def test_epilogue_layout_matches_header(tmp_path):
    """sizeof / offsetof of cimq_epilogue from gcc on include/cimq.h equal the ctypes mirror (as
    test_abi_host.test_struct_layouts_match_header does for the other structs)"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cimq.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(cimq_epilogue));', '  printf("relu %d\\n", CIMQ_EPI_RELU);']
    for fname, _ in L.Epilogue._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(cimq_epilogue, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in
               subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines() if line)
    assert int(got.pop("size")) == ctypes.sizeof(L.Epilogue)
    assert int(got.pop("relu")) == L.CIMQ_EPI_RELU
    assert [f for f, _ in L.Epilogue._fields_] == ["scale", "shift", "residual", "flags", "reserved"]
    for fname, v in got.items():
        assert int(v) == getattr(L.Epilogue, fname).offset, fname


# made-up device addresses: every refusal below is decided on the host before anything is dereferenced or
# launched (the calls return CIMQ_EINVAL; none reaches the null-pointer check that follows the refusals)
A = 0x7000_0000_0000


def _epi(scale=A + 0x100, shift=A + 0x200, residual=None, flags=0, reserved=0):
    e = L.Epilogue()
    e.scale, e.shift, e.residual, e.flags, e.reserved = scale, shift, residual, flags, reserved
    return e


def _call(lib, d, epi, out=A + 0x10_0000, beta=None, name="l1"):
    q = L.make_lsq_desc(-4, 3, 1e-3, 1e-3, 8)
    p = [A + 0x1000 * (i + 1) for i in range(7)]  # x, weight, alpha_act, alpha_weight, alpha_cim, bmask, signed
    return lib.cimq_module_forward_epilogue(ctypes.byref(d), ctypes.byref(q), p[0], p[1], p[2], p[3], p[4], beta, p[5],
                                            p[6], None if epi is None else ctypes.byref(epi), out, A + 0x40_0000,
                                            A + 0x80_0000, None)


def _refused(lib, rc, word):
    assert rc == L.CIMQ_EINVAL
    msg = lib.cimq_last_error()
    assert msg and word in msg, msg


@pytest.mark.parametrize("name", ["l1", "shift"])
def test_refuses_training_descriptor(lib, name):
    lib.cimq_module_route(None, None)  # leaves another message behind
    _refused(lib, _call(lib, case_desc(name, 0), _epi(), beta=A + 0x9000 if name == "shift" else None),
             b"CIMQ_OPT_INFERENCE")
    _refused(lib, _call(lib, case_desc(name, L.CIMQ_OPT_RECOMPUTE), _epi()), b"CIMQ_OPT_INFERENCE")


def test_refuses_null_epilogue_and_tables(lib):
    d = case_desc("l1", INF)
    _refused(lib, _call(lib, d, None), b"null")
    _refused(lib, _call(lib, d, _epi(scale=None)), b"null")
    _refused(lib, _call(lib, d, _epi(shift=None)), b"null")


def test_refuses_unknown_flags_and_reserved(lib):
    d = case_desc("l1", INF)
    for flags in (2, 4, 3, -1, 1 << 30):
        _refused(lib, _call(lib, d, _epi(flags=flags)), b"flags")
    _refused(lib, _call(lib, d, _epi(reserved=1)), b"reserved")
    _refused(lib, _call(lib, d, _epi(flags=L.CIMQ_EPI_RELU, reserved=-7)), b"reserved")


def test_refuses_misaligned_residual(lib):
    d = case_desc("l1", INF)
    for off in (4, 8, 12, 1):
        _refused(lib, _call(lib, d, _epi(residual=A + 0x20_0000 + off)), b"aligned")


@pytest.mark.parametrize("name", ["l1", "l2s2", "c48", "dense"])
def test_refuses_residual_overlapping_out(lib, name):
    d = case_desc(name, INF)
    Ho = (d.in_h + 2 * d.pad_h - d.kernel_h) // d.stride_h + 1
    nbytes = d.batch * d.out_channels * Ho * Ho * 4
    out = A + 0x10_0000
    for res in (out, out + 16, out + nbytes - 16, out - nbytes + 16):
        _refused(lib, _call(lib, d, _epi(residual=res), out=out), b"overlap")


def test_python_entry_refuses_differentiable_call():
    """functional.cim_module_conv_epilogue is forward only: with grad mode on and an argument that requires a
    gradient it raises before it touches a device"""
    from cim_quantization_amd import functional as F
    w = torch.zeros(16, 16, 3, 3, requires_grad=True)
    x = torch.zeros(1, 16, 8, 8)
    one = torch.ones(1)
    with pytest.raises(RuntimeError, match="forward only"):
        F.cim_module_conv_epilogue(x, w, one, one, None, torch.ones(1, 1, 3, 3, 1, 1), one, 1, 1, 1, 3, 1, 3, 1, 6,
                                   128, 8, torch.ones(16), torch.zeros(16))


def test_forward_fused_refuses_off_the_library_path():
    import cim_quantization_amd._modules as my_nn
    kw = dict(nbits_w=3, nbits_a=3, nbits_alpha=8, wbitslice=1, abitslice=1, xbar=128, adcbits=1.5, signed_xbar=True,
              stochastic_quant=False)
    x = torch.zeros(1, 16, 8, 8)
    s, t = torch.ones(16), torch.zeros(16)
    for m in (my_nn.Conv2dLSQCiM(16, 16, 3, 1, 1, bias=False, **kw),  # CPU tensors, first step not done
              my_nn.Conv2dLSQCiM(16, 16, 3, 1, 1, bias=True, **kw)):
        assert not m.fused_epilogue_ready(x)
        with pytest.raises(RuntimeError, match="forward_fused"):
            with torch.no_grad():
                m.forward_fused(x, s, t)


# ---------------------------------------------------------------------------------------------------
# BatchNorm folding
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [True, False])
def test_fold_bn_against_fp64(affine):
    """r = x * S + T with S = gamma / sqrt(var + eps), T = beta - mean * S in fp64.  The folded fp32 pair gives
    fl(fl(x * scale) + shift); four roundings separate it from r -- of scale, of shift, of the product, of the
    sum.  Each is at most 2^-24 relative to its own result: the first and third act on |x S|, the second on |T|,
    the fourth on at most |x S| + |T|, so the error is at most 3 * 2^-24 * (|x S| + |T|) to first order, and the
    bar leaves one more: |fl(fl(x scale) + shift) - r| <= 4 * 2^-24 * (|x S| + |T|) element-wise.  Derived, not
    measured (the largest ratio err / bound seen is 0.52)."""
    from cim_quantization_amd.harness.fuse import fold_bn
    g = torch.Generator().manual_seed(5)
    C = 64
    bn = torch.nn.BatchNorm2d(C, affine=affine).eval()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(C, generator=g) * 3)
        bn.running_var.copy_(torch.rand(C, generator=g) * 4 + 1e-3)
        if affine:
            bn.weight.copy_(torch.randn(C, generator=g))
            bn.bias.copy_(torch.randn(C, generator=g))
    scale, shift = fold_bn(bn)
    assert scale.dtype == shift.dtype == torch.float32 and scale.shape == shift.shape == (C,)
    gamma = bn.weight.detach().double() if affine else torch.ones(C, dtype=torch.float64)
    beta = bn.bias.detach().double() if affine else torch.zeros(C, dtype=torch.float64)
    S = gamma / torch.sqrt(bn.running_var.double() + bn.eps)
    T = beta - bn.running_mean.double() * S
    x = torch.randn(8, C, 5, 5, generator=g) * 4
    got = (x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)).double()
    xs = x.double() * S.view(1, -1, 1, 1)
    r = xs + T.view(1, -1, 1, 1)
    bound = 4 * 2.0 ** -24 * (xs.abs() + T.abs().view(1, -1, 1, 1))
    err = (got - r).abs()
    print("fold_bn: max err / bound =", float((err / bound).max()))
    assert bool((err <= bound).all())
    if not affine:  # gamma = 1, beta = 0
        assert torch.equal(scale, (1.0 / torch.sqrt(bn.running_var.double() + bn.eps)).float())


# ---------------------------------------------------------------------------------------------------
# FusedEval's wiring
# ---------------------------------------------------------------------------------------------------
def twin_forward(model, x, conv=lambda c, t: c(t)):
    """ResNet.forward with each BatchNorm replaced by its folded affine, written out: which shortcut, which
    order, which ReLU.  ``conv(module, input)``: how a conv is called."""
    from cim_quantization_amd.harness.fuse import fold_bn

    def cbr(c, bn, t, res=None):
        scale, shift = fold_bn(bn)
        y = conv(c, t) * scale.view(1, -1, 1, 1)
        y = y + shift.view(1, -1, 1, 1)
        if res is not None:
            y = y + res
        return torch.relu(y)

    y = cbr(model.conv1, model.bn1, x)
    for stage in (model.layer1, model.layer2, model.layer3):
        for blk in stage:
            z = cbr(blk.conv1, blk.bn1, y)
            y = cbr(blk.conv2, blk.bn2, z, blk.shortcut(y))
    y = torch.nn.functional.avg_pool2d(y, y.shape[3]).flatten(1)
    return model.linear(y)


def randomise_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.running_mean.copy_(torch.randn(n, generator=g) * 0.5)
                m.running_var.copy_(torch.rand(n, generator=g) + 0.5)
                m.weight.copy_(torch.randn(n, generator=g) * 0.5 + 1)
                m.bias.copy_(torch.randn(n, generator=g) * 0.3)


def test_fused_eval_wiring_cpu():
    from cim_quantization_amd.harness import models
    from cim_quantization_amd.harness.fuse import FusedEval
    torch.manual_seed(11)
    model = models.resnet20().eval()
    randomise_bn(model, 12)
    x = torch.randn(2, 3, 32, 32)
    fused = FusedEval(model)
    assert list(fused.parameters()) and all(a is b for a, b in zip(fused.parameters(), model.parameters()))
    with torch.no_grad():
        got = fused(x)
        want = twin_forward(model, x)
        assert torch.equal(got, want)
        # the tables are kept per BatchNorm and remade when one of its tensors changes
        t0 = fused.tables(model.bn1)
        assert fused.tables(model.bn1) is t0
        model.bn1.running_var.mul_(2.0)
        assert fused.tables(model.bn1) is not t0
        assert torch.equal(fused(x), twin_forward(model, x))
        assert not torch.equal(fused(x), got)


def test_fused_eval_refusals():
    from cim_quantization_amd.harness import models
    from cim_quantization_amd.harness.fuse import FusedEval
    model = models.resnet20().eval()
    x = torch.randn(1, 3, 32, 32)
    fused = FusedEval(model)
    with pytest.raises(RuntimeError, match="no_grad"):
        fused(x)
    model.layer2[1].bn2.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match="training mode"):
        fused(x)
    with pytest.raises(TypeError):
        FusedEval(torch.nn.Linear(2, 2))
