"""GPU: the ideal-ADC conv (Conv2dLSQCiM(adcbits=0) on cimq_ideal_forward / _backward, functional.cim_ideal_conv)
against a float64 reference: the module's two fp32 quantisers, then the conv and its autograd in float64.

Tolerances (tests/test_gpu_module_fused.py's convention): tensors within 1e-5 * max|ref| (+ 1e-12), the scalar
step-size gradients within 1e-5 * the sum of |terms| of their reductions, from the reference's intermediates."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle.cim_module_oracle import _gs, _rp

# (B, C, O, H, W, k, stride, pad, bits)
CASES = {
    "I1": (2, 16, 16, 8, 8, 3, 1, 1, 3),     # base: one tile, one block
    "I2": (2, 3, 32, 8, 8, 3, 1, 1, 8),      # SPLIT nibbles, C padded 3 -> 16, two output blocks
    "I3": (2, 24, 40, 6, 10, 3, 1, 1, 4),    # P = 60: masked m-tile tail, O and C no multiples of 16, rectangular
    "I4": (2, 32, 16, 9, 8, 3, 2, 1, 3),     # stride 2, odd height
    "I5": (3, 64, 64, 4, 4, 1, 1, 0, 2),     # 1x1, four output blocks, masked tiles
    "I6": (2, 6, 16, 14, 14, 5, 1, 0, 4),    # 25 taps (three tap groups in grad_w), no padding
    "I7": (2, 144, 16, 8, 8, 3, 1, 1, 4),    # contraction no multiple of 64 (one patch chunk)
    "I7c": (2, 1032, 16, 8, 8, 3, 1, 1, 4),  # ... raised to C = 1032: two patch chunks (test_ideal_host pins it)
    "I8": (5, 16, 16, 16, 16, 3, 1, 1, 3),   # four m-tiles per image, two grad_x bands, ten grad_w slabs
}


def make_case(name):
    B, C, O, H, W, k, s, p, bits = CASES[name]
    gen = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    x = torch.randn(B, C, H, W, generator=gen).relu()
    w = torch.empty(O, C, k, k)
    torch.nn.init.kaiming_normal_(w, generator=gen)
    qp_a, qn_w, qp_w = 2 ** bits - 1, -(2 ** (bits - 1)), 2 ** (bits - 1) - 1
    aa = (2 * x.abs().mean() / math.sqrt(qp_a)).reshape(1)   # the first-step formulas (lsq.py:532-542)
    aw = (2 * w.abs().mean() / math.sqrt(qp_w)).reshape(1)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    g = torch.randn(B, O, Ho, Wo, generator=gen)
    return dict(x=x, w=w, aa=aa, aw=aw, g=g, stride=(s, s), pad=(p, p), bits=bits, q=(qp_a, qn_w, qp_w))


def reference(c, bias=None):
    """out, gradients and the |terms| sums of the two step-size gradients, on the CPU."""
    qp_a, qn_w, qp_w = c["q"]
    x, w, aa, aw = (c[k].clone().requires_grad_(True) for k in ("x", "w", "aa", "aw"))
    ga, gw = 1.0 / math.sqrt(x.numel() * qp_a), 1.0 / math.sqrt(w.numel() * qp_w)
    sa, sw = _gs(aa, ga), _gs(aw, gw)
    ta, tw = x / sa, w / sw
    x_q, w_q = _rp(ta.clamp(0, qp_a)) * sa, _rp(tw.clamp(qn_w, qp_w)) * sw
    x_q.retain_grad()
    w_q.retain_grad()
    out = F.conv2d(x_q.double(), w_q.double(), None if bias is None else bias.double(), c["stride"], c["pad"])
    out.backward(c["g"].double())
    with torch.no_grad():
        def terms(t, dq, lo, hi, gs):
            inside = ((t >= lo) & (t <= hi)).double()
            return float((dq.double() * (t.clamp(lo, hi).round().double() - inside * t.double())).abs().sum() * gs)
        ta_terms, tw_terms = terms(ta, x_q.grad, 0, qp_a, ga), terms(tw, w_q.grad, qn_w, qp_w, gw)
    return out.detach(), x.grad, w.grad, aa.grad, aw.grad, ta_terms, tw_terms


def run_library(c, dev):
    from cim_quantization_amd.functional import cim_ideal_conv
    x, w, aa, aw = (c[k].to(dev).requires_grad_(True) for k in ("x", "w", "aa", "aw"))
    out = cim_ideal_conv(x, w, aa, aw, c["stride"], c["pad"], c["bits"], c["bits"])
    out.backward(c["g"].to(dev))
    torch.cuda.synchronize()
    return out.detach(), x.grad, w.grad, aa.grad, aw.grad


def close(name, mine, ref):
    ref = ref.double()
    err = float((mine.double().cpu() - ref).abs().max())
    bound = 1e-5 * float(ref.abs().max()) + 1e-12
    print(f"{name}: max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound, name


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_ideal_conv_vs_float64(cuda_device, name):
    c = make_case(name)
    out_r, gx_r, gw_r, ga_r, gaw_r, ta_terms, tw_terms = reference(c)
    out, gx, gw, ga, gaw = run_library(c, cuda_device)
    close("out", out, out_r)
    close("grad_x", gx, gx_r)
    close("grad_w", gw, gw_r)
    for what, mine, ref, terms in (("d alpha_act", ga, ga_r, ta_terms), ("d alpha_weight", gaw, gaw_r, tw_terms)):
        err = abs(float(mine) - float(ref))
        print(f"{what}: {float(mine):.6e} vs {float(ref):.6e}, err {err:.3e}, bound {1e-5 * terms:.3e}")
        assert err <= 1e-5 * terms + 1e-12, what


@pytest.mark.gpu
def test_ideal_backward_is_deterministic(cuda_device):
    c = make_case("I8")
    first, second = run_library(c, cuda_device), run_library(c, cuda_device)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("bias", [False, True])
def test_module_takes_the_library_path(cuda_device, bias):
    from cim_quantization_amd._modules.lsq import Conv2dLSQCiM
    c = make_case("I1")
    torch.manual_seed(5)
    m = Conv2dLSQCiM(16, 16, 3, stride=1, padding=1, bias=bias, nbits_w=3, nbits_a=3, adcbits=0).to(cuda_device)
    m.train()
    with torch.no_grad():
        m.weight.copy_(c["w"])
    x = c["x"].to(cuda_device)
    assert not m.ideal_ready(x)
    m(x)  # the initialising step runs on torch
    assert m.ideal_ready(x)
    with torch.no_grad():  # (make_case's step sizes to the bit: a device mean may round otherwise)
        m.alpha_act.copy_(c["aa"])
        m.alpha_weight.copy_(c["aw"])
    out = m(x)
    out.backward(c["g"].to(cuda_device))
    lib = run_library(c, cuda_device)
    if not bias:
        assert torch.equal(out.detach(), lib[0])
    for p, ref in ((m.weight, lib[2]), (m.alpha_act, lib[3]), (m.alpha_weight, lib[4])):
        assert torch.equal(p.grad.reshape(ref.shape), ref)
    if bias:
        b = m.bias.detach().cpu()
        close("out + bias", out.detach(), reference(c, bias=b)[0])
        close("d bias", m.bias.grad, c["g"].double().sum(dim=(0, 2, 3)))
    m.fused = False
    assert not m.ideal_ready(x)
