"""GPU: the ideal-ADC conv's large-layer forward (functional.cim_ideal_conv(wide_backward=True):
cim_ideal_fwd_wide_kernel) against tests/test_gpu_ideal.py's float64 reference within that file's tolerance
(1e-5 * max|ref|), and bit for bit against the unhinted call (cim_ideal_fwd_kernel), in training and no-grad calls."""
import math

import pytest
import torch

import cim_quantization_amd._lib as L
from test_gpu_ideal import close, reference

# (B, C, O, H, W, bits)
CASES = {
    "F1": (2, 128, 32, 8, 8, 3),     # one tile an image, W = 8, an output group narrower than a workgroup's span
    "F2": (2, 128, 64, 4, 32, 4),    # two tiles an image: the halo row is data on one side, zero on the other
    "F3": (3, 144, 32, 16, 16, 3),   # k-steps straddling taps, a partial last k-step, an odd batch, four tiles
    "F4": (2, 128, 320, 2, 32, 2),   # the resident-patch loop over two output groups, the second a tail
    "F5": (1, 640, 32, 2, 32, 3),    # two channel chunks: accumulators across chunks, restaging over a zero halo
}
_REF = {}


def case(name):
    """test_gpu_ideal_wide.make_case's recipe on this file's shapes; the float64 reference out computed once"""
    if name not in _REF:
        B, C, O, H, W, bits = CASES[name]
        gen = torch.Generator().manual_seed(3000 + sorted(CASES).index(name))
        x = torch.randn(B, C, H, W, generator=gen).relu()
        w = torch.empty(O, C, 3, 3)
        torch.nn.init.kaiming_normal_(w, generator=gen)
        qp_a, qn_w, qp_w = 2 ** bits - 1, -(2 ** (bits - 1)), 2 ** (bits - 1) - 1
        aa = (2 * x.abs().mean() / math.sqrt(qp_a)).reshape(1)
        aw = (2 * w.abs().mean() / math.sqrt(qp_w)).reshape(1)
        g = torch.randn(B, O, H, W, generator=gen)
        c = dict(x=x, w=w, aa=aa, aw=aw, g=g, stride=(1, 1), pad=(1, 1), bits=bits, q=(qp_a, qn_w, qp_w))
        _REF[name] = (c, reference(c)[0])
    return _REF[name]


def forward(c, dev, wide, train):
    from cim_quantization_amd.functional import cim_ideal_conv
    x, w, aa, aw = (c[k].to(dev).requires_grad_(train) for k in ("x", "w", "aa", "aw"))
    with torch.enable_grad() if train else torch.no_grad():
        out = cim_ideal_conv(x, w, aa, aw, c["stride"], c["pad"], c["bits"], c["bits"], wide_backward=wide)
    grads = ()
    if train:
        out.backward(c["g"].to(dev))
        grads = (x.grad, w.grad, aa.grad, aw.grad)
    torch.cuda.synchronize()
    return out.detach(), grads


@pytest.mark.gpu
@pytest.mark.parametrize("train", [True, False], ids=["train", "nograd"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_wide_forward(cuda_device, name, train):
    B, C, O, H, W, bits = CASES[name]
    opts = L.CIMQ_OPT_WIDE_BWD | (0 if train else L.CIMQ_OPT_INFERENCE)
    d = L.make_ideal_desc(B, C, H, W, O, 3, 3, (1, 1), (1, 1), bits, bits, options=opts)
    assert L.ideal_wide_fwd_plan(d)[0] == 1  # on the new kernel
    c, out_r = case(name)
    out, grads = forward(c, cuda_device, True, train)
    close("out", out, out_r)
    assert torch.equal(out, forward(c, cuda_device, False, train)[0])  # cim_ideal_fwd_kernel's bits
    if train:  # the backward pair reads what this forward left: two runs, the same bits
        for a, b in zip(grads, forward(c, cuda_device, True, True)[1]):
            assert torch.equal(a, b)


@pytest.mark.gpu
def test_module_evaluates_on_the_hint(cuda_device):
    from cim_quantization_amd._modules.lsq import Conv2dLSQCiM
    c, _ = case("F1")
    m = Conv2dLSQCiM(128, 32, 3, padding=1, bias=False, nbits_w=3, nbits_a=3, adcbits=0).to(cuda_device).train()
    x = c["x"].to(cuda_device)
    m(x)  # the initialising step runs on torch
    outs = []
    for hint in (True, False):
        m.wide_backward = hint
        with torch.no_grad():
            assert m.ideal_ready(x)
            outs.append(m(x))
    assert torch.equal(outs[0], outs[1])
