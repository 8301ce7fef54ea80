"""GPU: the output epilogue of the forward-only mode (cimq_module_forward_epilogue, ABI 16) on every forward
route -- per-channel affine, residual add and ReLU applied in the kernel that stores the output, bit for bit
equal to the four torch operations run one after another on the existing no-grad forward's output -- and the
layers above it: Conv2dLSQCiM.forward_fused, harness.fuse.FusedEval, validate(fused=True).
Shapes: test_inference_host.CASES (the smallest that reach each route) plus one with O = 24."""
import ctypes

import pytest
import torch

from test_epilogue_host import randomise_bn, twin_forward
from test_gpu_inference import _case, _check_route, _route0
from test_inference_host import CASES, INF

pytestmark = pytest.mark.gpu


def _F():
    from cim_quantization_amd import functional as F
    return F


def _L():
    import cim_quantization_amd._lib as L
    return L


def _plain(m, x):
    """the module's own no-grad forward: the value the kernels store today"""
    try:
        m.eval()
        with torch.no_grad():
            return m(x)
    finally:
        m.train()


def _fused(m, x, *a, **kw):
    try:
        m.eval()
        with torch.no_grad():
            return m.forward_fused(x, *a, **kw)
    finally:
        m.train()


def _ref(v, scale, shift, residual=None, relu=False):
    """the four torch operations, one after another (each one rounding)"""
    y = v * scale.view(1, -1, 1, 1)
    y = y + shift.view(1, -1, 1, 1)
    if residual is not None:
        y = y + residual
    return torch.relu(y) if relu else y


def _tables(v, seed):
    """random normal scale / shift, and a random normal residual scaled to the output so that ReLU cuts both ways"""
    g = torch.Generator().manual_seed(seed)
    O = v.shape[1]
    scale = torch.randn(O, generator=g).to(v.device)
    shift = (torch.randn(O, generator=g) * float(v.std())).to(v.device)
    res = (torch.randn(v.shape, generator=g) * float(v.std())).to(v.device)
    return scale, shift, res


@pytest.mark.parametrize("name", list(CASES))
def test_epilogue_bit_identity(cuda_device, name):
    m, x, _ = _case(name, cuda_device)
    _check_route(name, m, x)
    v = _plain(m, x)
    scale, shift, res = _tables(v, 100 + sum(map(ord, name)))
    for kw in (dict(), dict(relu=True), dict(residual=res, relu=True), dict(residual=res)):
        got = _fused(m, x, scale, shift, **kw)
        want = _ref(v, scale, shift, **kw)
        assert got.shape == v.shape and got.dtype == torch.float32
        assert torch.equal(got, want), (name, kw.keys(), float((got - want).abs().max()))
    relu_out = _ref(v, scale, shift, res, True)
    frac = float((relu_out == 0).float().mean())
    assert 0.05 < frac < 0.95, frac  # (ReLU does cut, and not everything)
    # the identity epilogue gives the plain output
    one, zero = torch.ones_like(scale), torch.zeros_like(shift)
    assert torch.equal(_fused(m, x, one, zero), v)
    # two calls with one set of buffers: bit-identical
    a = _fused(m, x, scale, shift, residual=res, relu=True)
    b = _fused(m, x, scale, shift, residual=res, relu=True)
    assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["l1", "conv1", "c48", "dense"])
def test_nan_in_residual_stays_nan(cuda_device, name):
    m, x, _ = _case(name, cuda_device)
    _check_route(name, m, x)
    v = _plain(m, x)
    scale, shift, res = _tables(v, 7)
    flat = res.view(-1)
    idx = torch.tensor([0, 5, flat.numel() // 2 + 3, flat.numel() - 1], device=res.device)
    flat[idx] = float("nan")
    got = _fused(m, x, scale, shift, residual=res, relu=True)
    assert torch.equal(torch.isnan(got), torch.isnan(res))
    assert int(torch.isnan(got).sum()) == 4
    want = _ref(v, scale, shift, res, True)
    ok = ~torch.isnan(res)
    assert torch.equal(got[ok], want[ok])


def test_channels_not_a_multiple_of_16(cuda_device):
    """O = 24 (C = 16, H = 16, w3a3, xbar 128): tables of exactly O elements, the channel guards of the route
    cimq_module_route reports for it (the general kernels: 24 is no power of two)"""
    import cim_quantization_amd._modules as my_nn
    torch.manual_seed(24)
    m = my_nn.Conv2dLSQCiM(16, 24, 3, 1, 1, bias=False, nbits_w=3, nbits_a=3, nbits_alpha=8, wbitslice=1, abitslice=1,
                           xbar=128, adcbits=1.5, signed_xbar=True, stochastic_quant=False)
    torch.nn.init.kaiming_normal_(m.weight)
    m = m.to(cuda_device).train()
    x = torch.randn(2, 16, 16, 16, generator=torch.Generator().manual_seed(25)).relu().to(cuda_device)
    m(x)
    assert _route0(m, x) == "general"
    v = _plain(m, x)
    assert v.shape == (2, 24, 16, 16)
    scale, shift, res = _tables(v, 26)
    assert scale.numel() == shift.numel() == 24
    for kw in (dict(), dict(relu=True), dict(residual=res, relu=True)):
        assert torch.equal(_fused(m, x, scale, shift, **kw), _ref(v, scale, shift, **kw)), kw.keys()


def _raw_epi(m, x, scale, shift, res, relu, out=None):
    """cimq_module_forward_epilogue through ctypes on module m's parameters"""
    F, L = _F(), _L()
    dev = x.device
    desc, lsq = F.module_descs(m, tuple(x.shape))
    desc.options = INF
    sizes = L.query_sizes(desc)
    B, O = x.shape[0], m.weight.shape[0]
    Ho = (x.shape[2] + 2 * m.padding[0] - m.weight.shape[2]) // m.stride[0] + 1
    if out is None:
        out = torch.empty(B, O, Ho, Ho, device=dev)
    cbuf = torch.empty(max(sizes.ctx_bytes, 1), device=dev, dtype=torch.uint8)
    ws = torch.empty(max(sizes.fwd_workspace_bytes, 1), device=dev, dtype=torch.uint8)
    t = [x.contiguous(), m.weight.detach().contiguous(), m.alpha_act.detach().reshape(-1)[:1].contiguous(),
         m.alpha_weight.detach().reshape(-1)[:1].contiguous(),
         None if m.alpha_cim is None else m.alpha_cim.detach().contiguous(),
         m.beta_cim.detach().contiguous() if m.adc_shift else None,
         m.binary_mask.to(device=dev, dtype=torch.int8).contiguous(),
         m.signed_act.detach().to(torch.float32).reshape(-1)[:1].contiguous()]
    p = lambda u: None if u is None else u.data_ptr()  # noqa: E731
    epi = L.make_epilogue(p(scale), p(shift), p(res), relu)
    rc = L.load().cimq_module_forward_epilogue(desc, lsq, *[p(u) for u in t], ctypes.byref(epi), p(out), p(cbuf), p(ws),
                                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("name", ["l1", "conv1", "c48", "dense", "shift"])
def test_raw_abi(cuda_device, name):
    """one call per route family (fwd5, v3, general, dense, the shift ADC on v3) straight through the C ABI"""
    L = _L()
    m, x, _ = _case(name, cuda_device)
    _check_route(name, m, x)
    v = _plain(m, x)
    scale, shift, res = _tables(v, 300 + sum(map(ord, name)))
    rc, out = _raw_epi(m, x, scale, shift, res, True)
    assert rc == 0, L.load().cimq_last_error()
    assert torch.equal(out, _ref(v, scale, shift, res, True))
    rc, out = _raw_epi(m, x, scale, shift, None, False)
    assert rc == 0, L.load().cimq_last_error()
    assert torch.equal(out, _ref(v, scale, shift))
    # a residual overlapping out is refused with real buffers too, and nothing is written
    both = torch.full((2 * v.numel() - 4,), 7.0, device=v.device)
    rc, _ = _raw_epi(m, x, scale, shift, both[v.numel() - 4:], True, out=both[:v.numel()].view(v.shape))
    assert rc == L.CIMQ_EINVAL and b"overlap" in L.load().cimq_last_error()
    assert bool((both == 7.0).all())


def test_forward_fused_keeps_inference_weights(cuda_device):
    m, x, _ = _case("l1", cuda_device)
    v = _plain(m, x)
    scale, shift, res = _tables(v, 9)
    try:
        m.eval()
        m._inf_prep = None
        with torch.no_grad():
            a = m.forward_fused(x, scale, shift, relu=True)
            prep = m._inf_prep
            assert prep is not None
            b = m.forward_fused(x, scale, shift, residual=res, relu=True)
            assert m._inf_prep is prep and m._inf_prep.buf is prep.buf
            m(x)  # ... and the plain forward shares it
            assert m._inf_prep is prep
        assert torch.equal(a, _ref(v, scale, shift, None, True))
        assert torch.equal(b, _ref(v, scale, shift, res, True))
        # a residual that is neither contiguous nor fp32 is made so
        r2 = res.double().transpose(2, 3).contiguous().transpose(2, 3)
        assert not r2.is_contiguous()
        with torch.no_grad():
            c = m.forward_fused(x, scale, shift, residual=r2, relu=True)
        assert torch.equal(c, b)
        with pytest.raises(RuntimeError, match="forward only"):
            m.forward_fused(x.clone().requires_grad_(True), scale, shift)
    finally:
        m.train()


# ---------------------------------------------------------------------------------------------------
# the whole network
# ---------------------------------------------------------------------------------------------------
_NET = {}


def _net(dev):
    """harness resnet20 through ReplaceModuleTool with cfg2's settings (w3a3, xbar 128, adc 1.5, first conv w8a8)
    at B = 2, one training-mode forward for the first-step initialisation, then eval()"""
    if "m" in _NET:
        return _NET["m"], _NET["x"]
    from cim_quantization_amd._modules.lsq import Conv2dLSQCiM
    from cim_quantization_amd.harness import models
    from cim_quantization_amd.harness.replace import ReplaceModuleTool
    torch.manual_seed(2020)
    model = models.resnet20()
    ReplaceModuleTool(model, {"Conv2d": [Conv2dLSQCiM]}, True, nbits_w=3, nbits_a=3, nbits_alpha=8, wbitslice=1,
                      abitslice=1, xbar=128, adcbits=1.5, signed_xbar=True, stochastic_quant=False).replace()
    model = model.to(dev).train()
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(2021)).to(dev)
    model(x)
    randomise_bn(model, 2022)
    model.eval()
    _NET["m"], _NET["x"] = model, x
    return model, x


def _own_forward(c, t):
    with torch.no_grad():
        return c(t)


def test_fused_eval_resnet20(cuda_device):
    from cim_quantization_amd._modules.lsq import Conv2dLSQCiM
    from cim_quantization_amd.harness.fuse import FusedEval
    model, x = _net(cuda_device)
    convs = [m for m in model.modules() if isinstance(m, Conv2dLSQCiM)]
    assert len(convs) == 19 and model.conv1.nbits_w == 8 and convs[1].nbits_w == 3
    with torch.no_grad():
        assert all(c.fused_epilogue_ready(torch.empty(1, c.in_channels, 8, 8, device=cuda_device)) for c in convs)
        got = FusedEval(model)(x)
        want = twin_forward(model, x, _own_forward)
        assert torch.equal(got, want)
        bn = model(x)
    # against the BatchNorm path itself no tolerance can be derived (a last-bit difference in front of a
    # quantiser can move an activation code): recorded in DESIGN.md section 7, not asserted
    print("fused vs BatchNorm path: max |logit difference| = %.3e (max |logit| %.3e)"
          % (float((got - bn).abs().max()), float(bn.abs().max())))


def test_validate_fused(cuda_device):
    from cim_quantization_amd.harness import train
    model, x = _net(cuda_device)
    g = torch.Generator().manual_seed(5)
    batches = [(torch.randn(2, 3, 32, 32, generator=g).to(cuda_device), torch.randint(0, 10, (2,), generator=g).to(cuda_device))
               for _ in range(3)]

    class HP:
        overfit_test = False

    crit = torch.nn.CrossEntropyLoss()
    got = train.validate(batches, model, crit, HP, fused=True)

    class Twin(torch.nn.Module):
        def __init__(self, model):
            super().__init__()
            self.model = model

        def forward(self, t):
            return twin_forward(self.model, t, _own_forward)

    want = train.validate(batches, Twin(model), crit, HP)
    assert got == want
    assert len(got) == 3 and 0.0 <= got[0] <= got[1] <= 100.0
