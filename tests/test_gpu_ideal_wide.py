"""GPU: the ideal-ADC conv's large-layer backward (functional.cim_ideal_conv(wide_backward=True):
cim_ideal_gx_wide_kernel + cim_ideal_gw_wide_kernel) against tests/test_gpu_ideal.py's float64 reference, within that
file's tolerances: tensors within 1e-5 * max|ref|, the step-size gradients within 1e-5 * the sum of |terms|."""
import math

import pytest
import torch

from test_gpu_ideal import close, reference

# (B, C, O, H, W, bits)
CASES = {
    "W1": (2, 128, 32, 8, 8, 3),     # one tile; W = 8, a segment is a whole row
    "W2": (2, 128, 64, 4, 32, 4),    # two tiles an image: the halo row is data on one side, zero on the other
    "W3": (3, 144, 32, 16, 16, 3),   # a channel-tile tail in both kernels, an odd batch
    "W4": (2, 128, 256, 2, 32, 2),   # four grad_x output chunks, four grad_w output tiles
    "W5": (2, 128, 32, 8, 8, 8),     # codes up to 255
    "W6": (5, 128, 32, 16, 16, 3),   # four stages per slab, five slabs (test_ideal_wide_host pins the counts)
}


def make_case(name):
    B, C, O, H, W, bits = CASES[name]
    gen = torch.Generator().manual_seed(2000 + sorted(CASES).index(name))
    x = torch.randn(B, C, H, W, generator=gen).relu()
    w = torch.empty(O, C, 3, 3)
    torch.nn.init.kaiming_normal_(w, generator=gen)
    qp_a, qn_w, qp_w = 2 ** bits - 1, -(2 ** (bits - 1)), 2 ** (bits - 1) - 1
    aa = (2 * x.abs().mean() / math.sqrt(qp_a)).reshape(1)
    aw = (2 * w.abs().mean() / math.sqrt(qp_w)).reshape(1)
    g = torch.randn(B, O, H, W, generator=gen)
    return dict(x=x, w=w, aa=aa, aw=aw, g=g, stride=(1, 1), pad=(1, 1), bits=bits, q=(qp_a, qn_w, qp_w))


def run_library(c, dev, wide):
    from cim_quantization_amd.functional import cim_ideal_conv
    x, w, aa, aw = (c[k].to(dev).requires_grad_(True) for k in ("x", "w", "aa", "aw"))
    out = cim_ideal_conv(x, w, aa, aw, c["stride"], c["pad"], c["bits"], c["bits"], wide_backward=wide)
    out.backward(c["g"].to(dev))
    torch.cuda.synchronize()
    return out.detach(), x.grad, w.grad, aa.grad, aw.grad


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_wide_backward_vs_float64(cuda_device, name):
    c = make_case(name)
    out_r, gx_r, gw_r, ga_r, gaw_r, ta_terms, tw_terms = reference(c)
    out, gx, gw, ga, gaw = run_library(c, cuda_device, True)
    assert torch.equal(out, run_library(c, cuda_device, False)[0])  # the same forward
    close("out", out, out_r)
    close("grad_x", gx, gx_r)
    close("grad_w", gw, gw_r)
    for what, mine, ref, terms in (("d alpha_act", ga, ga_r, ta_terms), ("d alpha_weight", gaw, gaw_r, tw_terms)):
        err = abs(float(mine) - float(ref))
        print(f"{what}: {float(mine):.6e} vs {float(ref):.6e}, err {err:.3e}, bound {1e-5 * terms:.3e}")
        assert err <= 1e-5 * terms + 1e-12, what
    if name == "W6":  # multi-slab: two runs, the same bits
        for a, b in zip((out, gx, gw, ga, gaw), run_library(c, cuda_device, True)):
            assert torch.equal(a, b)


@pytest.mark.gpu
def test_module_passes_the_hint(cuda_device):
    from cim_quantization_amd._modules.lsq import Conv2dLSQCiM
    c = make_case("W1")
    m = Conv2dLSQCiM(128, 32, 3, padding=1, bias=False, nbits_w=3, nbits_a=3, adcbits=0).to(cuda_device).train()
    m.wide_backward = True
    with torch.no_grad():
        m.weight.copy_(c["w"])
    x = c["x"].to(cuda_device)
    m(x)  # the initialising step runs on torch
    assert m.ideal_ready(x)
    with torch.no_grad():
        m.alpha_act.copy_(c["aa"])
        m.alpha_weight.copy_(c["aw"])
    m(x).backward(c["g"].to(cuda_device))
    lib = run_library(c, cuda_device, True)
    for p, ref in ((m.weight, lib[2]), (m.alpha_act, lib[3]), (m.alpha_weight, lib[4])):
        assert torch.equal(p.grad.reshape(ref.shape), ref)
