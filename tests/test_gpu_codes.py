"""GPU: activation codes between convs (cimq_module_forward_codes, ABI 16 minor 1) on every forward route -- the
codes a kernel's epilogue writes equal the torch twin applied to the float epilogue's output, a layer fed the
twin's codes gives the output it gives on the fp32 tensor, producer -> consumer chains through codes equal the
chains through fp32, and FusedEval(model, codes=True) gives FusedEval(model)'s logits.  Every comparison is
torch.equal.  The twin's division runs on the CPU (IEEE), as the kernels' does.
Shapes: test_inference_host.CASES (the smallest that reach each route) plus O = 24 and one 12 x 32 image."""
import ctypes

import pytest
import torch

from test_gpu_epilogue import _fused, _net, _plain, _tables
from test_gpu_inference import _case, _check_route, _route0
from test_inference_host import CASES, INF

pytestmark = pytest.mark.gpu

KW = dict(nbits_w=3, nbits_a=3, nbits_alpha=8, wbitslice=1, abitslice=1, xbar=128, adcbits=1.5, signed_xbar=True,
          stochastic_quant=False)


def _F():
    from cim_quantization_amd import functional as F
    return F


def _L():
    import cim_quantization_amd._lib as L
    return L


def _ready(m, x):
    try:
        m.eval()
        return m.codes_ready(x)
    finally:
        m.train()


def _consumer(channels, dev, alpha, nbits=3):
    """a layer that reads ``channels`` channels, with its activation step-size parameter set: the codes are for it"""
    import cim_quantization_amd._modules as my_nn
    kw = dict(KW, nbits_a=nbits)
    c = my_nn.Conv2dLSQCiM(channels, 16, 3, 1, 1, bias=False, **kw).to(dev)
    with torch.no_grad():
        c.alpha_act.fill_(float(alpha))
    return c


def _twin(cons, y):
    """the consumer's codes of y, the division on the host"""
    return cons.act_codes(y.detach().cpu())


def _o24(dev):
    import cim_quantization_amd._modules as my_nn
    if "o24" not in _O24:
        torch.manual_seed(24)
        m = my_nn.Conv2dLSQCiM(16, 24, 3, 1, 1, bias=False, **KW)
        torch.nn.init.kaiming_normal_(m.weight)
        m = m.to(dev).train()
        x = torch.randn(2, 16, 16, 16, generator=torch.Generator().manual_seed(25)).relu().to(dev)
        m(x)
        _O24["o24"] = (m, x)
    return _O24["o24"]


_O24 = {}
OUT_CASES = [n for n in CASES if CASES[n][-1] in ("fwd5", "v3", "general")] + ["o24"]
IN_CASES = [n for n in CASES if n != "conv1"]


def _get(name, dev):
    if name == "o24":
        m, x = _o24(dev)
        assert _route0(m, x) == "general"
        return m, x
    m, x, _ = _case(name, dev)
    _check_route(name, m, x)
    return m, x


def _plant_nans(t):
    flat = t.view(-1)
    idx = torch.tensor([0, 5, flat.numel() // 2 + 3, flat.numel() - 1], device=t.device)
    flat[idx] = float("nan")
    return idx


# ---------------------------------------------------------------------------------------------------
# 1. output codes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OUT_CASES)
def test_output_codes(cuda_device, name):
    m, x = _get(name, cuda_device)
    assert _ready(m, x)[1]
    v = _plain(m, x)
    scale, shift, res = _tables(v, 500 + sum(map(ord, name)))
    ep = dict(residual=res, relu=True)
    y = _fused(m, x, scale, shift, **ep)  # the float epilogue (proven against torch by test_gpu_epilogue)
    # the consumer's step size from a quantile of the positive outputs: Qp - 0.5 steps reach their 92 % point, so
    # a few per cent of the codes sit at Qp and every code below occurs
    qp = 7
    pos = y[y > 0].float().cpu()
    cons = _consumer(v.shape[1], cuda_device, float(torch.quantile(pos[:1_000_000], 0.92)) / (qp - 0.5))
    want = _twin(cons, y)
    frac0, fracq = float((want == 0).float().mean()), float((want == qp).float().mean())
    print(f"{name}: codes 0: {frac0:.3f}, codes Qp: {fracq:.3f}, present {sorted(set(want.view(-1).tolist()))}")
    assert set(want.view(-1).tolist()) == set(range(qp + 1))
    assert 0.05 < frac0 < 0.80 and fracq >= 0.01
    yf, q = _fused(m, x, scale, shift, out_quant=cons, **ep)
    assert q.dtype == torch.uint8 and q.shape == y.shape and q.is_contiguous()
    assert torch.equal(yf, y)
    assert torch.equal(q.cpu(), want)
    q2 = _fused(m, x, scale, shift, out_quant=cons, keep_float=False, **ep)
    assert torch.is_tensor(q2) and q2.dtype == torch.uint8
    assert torch.equal(q2.cpu(), want)
    # without ReLU and residual too (negative values clamp to code 0)
    y3 = _fused(m, x, scale, shift)
    assert torch.equal(_fused(m, x, scale, shift, out_quant=cons, keep_float=False).cpu(), _twin(cons, y3))


@pytest.mark.parametrize("name", OUT_CASES)
def test_output_codes_ties_round_to_even(cuda_device, name):
    """exact .5 ties: a power-of-two alpha_act (the step size is then alpha_act itself), shift 0, and one channel
    with scale 0 whose residual holds (k + 0.5) * alpha_act for k = 0 .. Qp + 1 -- the stored value is the residual
    exactly, and its quotient by the step size is exactly k + 0.5"""
    m, x = _get(name, cuda_device)
    v = _plain(m, x)
    scale, _, res = _tables(v, 77)
    shift = torch.zeros_like(scale)
    alpha, qp = 0.25, 7
    cons = _consumer(v.shape[1], cuda_device, alpha)
    scale[0] = 0.0
    n = res[:, 0].numel()
    k = torch.arange(n, device=res.device) % (qp + 2)
    res[:, 0] = ((k.float() + 0.5) * alpha).view(res[:, 0].shape)
    y = _fused(m, x, scale, shift, residual=res)
    yc = y.cpu()
    sa = _F().act_code_step(*cons._code_quant(y.numel())[:2]).cpu()
    assert float(sa) == alpha
    quo = yc / sa
    ties = (quo - torch.floor(quo)) == 0.5
    assert int(ties.sum()) >= 1 and bool(ties[:, 0].all())
    want = _twin(cons, y)
    assert want[0, 0].reshape(-1)[:9].tolist() == [0, 2, 2, 4, 4, 6, 6, 7, 7]  # ties to even, then the clamp
    q = _fused(m, x, scale, shift, residual=res, out_quant=cons, keep_float=False)
    assert torch.equal(q.cpu(), want)


@pytest.mark.parametrize("name", OUT_CASES)
def test_output_codes_nan(cuda_device, name):
    """four NaNs in the residual give code Qp + 1 exactly there"""
    m, x = _get(name, cuda_device)
    v = _plain(m, x)
    scale, shift, res = _tables(v, 7)
    _plant_nans(res)
    cons = _consumer(v.shape[1], cuda_device, float(v.abs().mean()))
    qp = 2 ** cons.nbits_a - 1
    y, q = _fused(m, x, scale, shift, residual=res, relu=True, out_quant=cons)
    assert torch.equal(torch.isnan(y), torch.isnan(res))
    assert torch.equal(q == qp + 1, torch.isnan(res)) and int((q == qp + 1).sum()) == 4
    assert torch.equal(q.cpu(), _twin(cons, y))


# ---------------------------------------------------------------------------------------------------
# 2. input codes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IN_CASES)
def test_input_codes(cuda_device, name):
    m, x = _get(name, cuda_device)
    assert _ready(m, x)[0]
    scale, shift, res = _tables(_plain(m, x), 600 + sum(map(ord, name)))
    qp = 2 ** m.nbits_a - 1
    for nans in (False, True):
        xx = x.clone()
        if nans:
            _plant_nans(xx)
        xq = m.act_codes(xx.cpu()).to(cuda_device)
        assert int(xq.max()) == (qp + 1 if nans else qp)  # (no byte above Qp + 1 is fed)
        assert int((xq == qp + 1).sum()) == (4 if nans else 0)
        for ep in (dict(), dict(residual=res, relu=True)):
            want = _fused(m, xx, scale, shift, **ep)
            got = _fused(m, xq, scale, shift, **ep)
            assert got.dtype == torch.float32 and got.shape == want.shape
            # (bit for bit, a NaN in the output included)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (name, nans, ep.keys())


def test_input_codes_rectangular(cuda_device):
    """16 -> 16 channels on a 12 x 32 image, B = 1 (rows and columns differ in the staging's index arithmetic)"""
    import cim_quantization_amd._modules as my_nn
    torch.manual_seed(1232)
    m = my_nn.Conv2dLSQCiM(16, 16, 3, 1, 1, bias=False, **KW)
    torch.nn.init.kaiming_normal_(m.weight)
    m = m.to(cuda_device).train()
    x = torch.randn(1, 16, 12, 32, generator=torch.Generator().manual_seed(1233)).relu().to(cuda_device)
    m(x)
    assert _ready(m, x) == (True, True)
    v = _plain(m, x)
    scale, shift, res = _tables(v, 1234)
    xq = m.act_codes(x.cpu()).to(cuda_device)
    want = _fused(m, x, scale, shift, residual=res, relu=True)
    assert torch.equal(_fused(m, xq, scale, shift, residual=res, relu=True), want)
    cons = _consumer(16, cuda_device, float(want[want > 0].mean()) / 2)
    q = _fused(m, xq, scale, shift, residual=res, relu=True, out_quant=cons, keep_float=False)
    assert torch.equal(q.cpu(), _twin(cons, want))


@pytest.mark.parametrize("name,C,H,nba", [("oddw", 3, 15, 3), ("a5", 16, 16, 5)])
def test_input_codes_prologue_paths(cuda_device, name, C, H, nba):
    """the two paths of the code-reading prologue that no CASES entry takes: its element-wise tail (3 x 15 x 15
    elements: not a multiple of 4) and its 8-byte slice words (5-bit activations, Qp = 31)"""
    import cim_quantization_amd._modules as my_nn
    torch.manual_seed(1500 + nba + H)
    m = my_nn.Conv2dLSQCiM(C, 16, 3, 1, 1, bias=False, **dict(KW, nbits_a=nba))
    torch.nn.init.kaiming_normal_(m.weight)
    m = m.to(cuda_device).train()
    x = torch.randn(1, C, H, H, generator=torch.Generator().manual_seed(1501)).relu().to(cuda_device)
    m(x)
    x = x * 1.5  # (past the step size the first step chose, so that the clamp at Qp is reached)
    assert _ready(m, x)[0]
    assert (x.numel() % 4 != 0) == (name == "oddw")
    scale, shift, res = _tables(_plain(m, x), 1502)
    qp = 2 ** nba - 1
    for nans in (False, True):
        xx = x.clone()
        if nans:
            _plant_nans(xx)
        xq = m.act_codes(xx.cpu()).to(cuda_device)
        assert int(xq.max()) == (qp + 1 if nans else qp)
        want = _fused(m, xx, scale, shift, residual=res, relu=True)
        got = _fused(m, xq, scale, shift, residual=res, relu=True)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (name, nans)


# ---------------------------------------------------------------------------------------------------
# 3. chains
# ---------------------------------------------------------------------------------------------------
class _Raw:
    """cimq_module_forward_codes through ctypes on module m's parameters, with ONE set of buffers (out, out_codes,
    ctx, workspace) for every call it makes"""

    def __init__(self, m, x_shape):
        F, L = _F(), _L()
        dev = m.weight.device
        self.m, self.dev = m, dev
        self.desc, self.lsq = F._module_descs(tuple(x_shape), m.weight, m.stride, m.padding, m.dilation, m.nbits_a,
                                              m.abitslice, m.nbits_w, m.wbitslice, m.adcbits, m.xbar, m.nbits_alpha,
                                              m.alpha_cim is not None, False)
        self.desc.options = INF
        sizes = L.query_sizes(self.desc)
        ho = (x_shape[2] + 2 * m.padding[0] - m.weight.shape[2]) // m.stride[0] + 1
        wo = (x_shape[3] + 2 * m.padding[1] - m.weight.shape[3]) // m.stride[1] + 1
        self.out = torch.full((x_shape[0], m.out_channels, ho, wo), 7.0, device=dev)
        self.oq = torch.zeros(self.out.shape, device=dev, dtype=torch.uint8)
        self.cbuf = torch.empty(max(sizes.ctx_bytes, 1), device=dev, dtype=torch.uint8)
        self.ws = torch.empty(max(sizes.fwd_workspace_bytes, 1), device=dev, dtype=torch.uint8)
        self.t = [m.weight.detach().contiguous(), m.alpha_act.detach().reshape(-1)[:1].contiguous(),
                  m.alpha_weight.detach().reshape(-1)[:1].contiguous(),
                  None if m.alpha_cim is None else m.alpha_cim.detach().contiguous(), None,
                  m.binary_mask.to(device=dev, dtype=torch.int8).contiguous(),
                  m.signed_act.detach().to(torch.float32).reshape(-1)[:1].contiguous()]

    def call(self, scale, shift, res, relu, x=None, x_codes=None, cons=None, no_float=False, out=True):
        """``cons``: the consumer layer the codes in self.oq are for (None: no out_codes); ``out`` False: NULL"""
        L = _L()
        p = lambda u: None if u is None else u.data_ptr()  # noqa: E731
        epi = L.make_epilogue(p(scale), p(shift), p(res), relu)
        if cons is None:
            io = L.make_act_codes(x_codes=p(x_codes))
        else:
            alpha, gs, qp = cons._code_quant(self.out.numel())
            oa = alpha.detach().reshape(-1)[:1].contiguous()
            io = L.make_act_codes(p(x_codes), p(self.oq), p(oa), gs, qp, no_float)
        rc = L.load().cimq_module_forward_codes(self.desc, self.lsq, ctypes.byref(io), p(x), *[p(u) for u in self.t],
                                                ctypes.byref(epi), p(self.out) if out else None, p(self.cbuf),
                                                p(self.ws), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0, L.load().cimq_last_error()


def _second(name, dev, batch):
    """the consumer of a chain: the case's module (a fresh one where the producer is the same case, so that the
    two layers differ), initialised on an input of the chain's batch size"""
    import cim_quantization_amd._modules as my_nn
    B, C, O, H, s, nb, xbar, adc, k, p, _ = CASES[name]
    torch.manual_seed(900 + sum(map(ord, name)))
    kw = dict(KW, nbits_w=nb, nbits_a=nb, xbar=xbar, adcbits=adc)
    m = my_nn.Conv2dLSQCiM(C, O, k, s, p, bias=False, **kw)
    torch.nn.init.kaiming_normal_(m.weight)
    m = m.to(dev).train()
    m(torch.randn(batch, C, H, H, generator=torch.Generator().manual_seed(901)).relu().to(dev))
    return m


@pytest.mark.parametrize("prod,cons", [("l1", "l1"), ("l2s2", "l2"), ("l3", "l3"), ("conv1", "l1"), ("c48", "c48")])
def test_chain(cuda_device, prod, cons):
    m1, x = _get(prod, cuda_device)
    m2 = _second(cons, cuda_device, x.shape[0])
    v1 = _plain(m1, x)
    s1, t1, _ = _tables(v1, 40)
    y1 = _fused(m1, x, s1, t1, relu=True)
    assert tuple(y1.shape[1:]) == (CASES[cons][1], CASES[cons][3], CASES[cons][3])
    with torch.no_grad():  # (the consumer's step size to the scale of what it is fed)
        m2.alpha_act.fill_(float(y1[y1 > 0].mean()) / 2)
    assert _ready(m1, x)[1] and _ready(m2, y1)[0]
    v2 = _plain(m2, y1)
    s2, t2, r2res = _tables(v2, 41)
    want = _fused(m2, y1, s2, t2, residual=r2res, relu=True)  # through the producer's float epilogue
    runs = []
    for _ in range(2):
        yf, q = _fused(m1, x, s1, t1, relu=True, out_quant=m2)
        assert torch.equal(yf, y1)
        q_only = _fused(m1, x, s1, t1, relu=True, out_quant=m2, keep_float=False)
        assert torch.equal(q_only, q)
        runs.append(_fused(m2, q_only, s2, t2, residual=r2res, relu=True))
    assert torch.equal(runs[0], want) and torch.equal(runs[1], want)
    assert torch.equal(q.cpu(), m2.act_codes(y1.cpu()))
    # two runs of the raw calls on one set of buffers (producer: out, codes, ctx, workspace; consumer: out, ctx,
    # workspace) are equal, and equal to the above
    try:
        m1.eval()
        m2.eval()
        r1, r2 = _Raw(m1, x.shape), _Raw(m2, y1.shape)
        snaps = []
        for _ in range(2):
            r1.call(s1, t1, None, True, x=x, cons=m2)
            r2.call(s2, t2, r2res, True, x_codes=r1.oq)
            snaps.append((r1.out.clone(), r1.oq.clone(), r2.out.clone()))
    finally:
        m1.train()
        m2.train()
    for a, b in zip(snaps[0], snaps[1]):
        assert torch.equal(a, b)
    assert torch.equal(snaps[0][0], y1) and torch.equal(snaps[0][1], q) and torch.equal(snaps[0][2], want)


# ---------------------------------------------------------------------------------------------------
# 4. the whole network
# ---------------------------------------------------------------------------------------------------
def test_fused_eval_codes_resnet20(cuda_device):
    from cim_quantization_amd.harness.fuse import FusedEval
    model, x = _net(cuda_device)
    with torch.no_grad():
        want = FusedEval(model)(x)
        fused = FusedEval(model, codes=True)
        got = fused(x)
        assert torch.equal(got, want)
        assert torch.equal(fused(x), want)
    edges = fused.code_edges
    assert len(edges) == 18 and len({e[1] for e in edges}) == 18  # the inputs of 18 of the 19 convs
    assert edges[0] == ("conv1", "layer1.0.conv1", "float+codes")
    assert edges[1] == ("layer1.0.conv1", "layer1.0.conv2", "codes")
    assert [e[2] for e in edges].count("codes") == 9
    assert "conv1" not in {e[1] for e in edges}
    # a conv that leaves the library path after codes were planned for it: asked again on every forward, so the
    # edges into and out of it go back to fp32 and the logits are still FusedEval(model)'s
    c = model.layer1[0].conv2
    try:
        c.fused = False
        with torch.no_grad():
            assert torch.equal(fused(x), FusedEval(model)(x))
        assert len(fused.code_edges) == 16 and all("layer1.0.conv2" not in e[:2] for e in fused.code_edges)
    finally:
        c.fused = True
    with torch.no_grad():
        assert torch.equal(fused(x), want) and len(fused.code_edges) == 18


def test_validate_fused_codes(cuda_device):
    from cim_quantization_amd.harness import train
    model, x = _net(cuda_device)
    g = torch.Generator().manual_seed(5)
    batches = [(torch.randn(2, 3, 32, 32, generator=g).to(cuda_device), torch.randint(0, 10, (2,), generator=g).to(cuda_device))
               for _ in range(3)]

    class HP:
        overfit_test = False

    crit = torch.nn.CrossEntropyLoss()
    assert train.validate(batches, model, crit, HP, fused=True, codes=True) == train.validate(batches, model, crit, HP,
                                                                                              fused=True)
    with pytest.raises(ValueError):
        train.validate(batches, model, crit, HP, codes=True)


# ---------------------------------------------------------------------------------------------------
# 5. the raw C ABI
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["l1", "w2a2", "c48"])
def test_raw_abi(cuda_device, name):
    """cimq_module_forward_codes through ctypes: x = NULL with x_codes, and with CIMQ_CODES_NO_FLOAT out = NULL"""
    m, x = _get(name, cuda_device)
    dev = x.device
    v = _plain(m, x)
    scale, shift, res = _tables(v, 300 + sum(map(ord, name)))
    cons = _consumer(v.shape[1], cuda_device, float(v.abs().mean()))
    want = _fused(m, x, scale, shift, residual=res, relu=True)
    xq = m.act_codes(x.cpu()).to(dev)
    r = _Raw(m, x.shape)
    r.call(scale, shift, res, True, x_codes=xq)  # codes in, x = NULL
    assert torch.equal(r.out, want)
    r.out.fill_(7.0)
    r.call(scale, shift, res, True, x_codes=xq, cons=cons, no_float=True, out=False)  # codes in and out, out = NULL
    assert torch.equal(r.oq.cpu(), _twin(cons, want)) and bool((r.out == 7.0).all())
    r.oq.zero_()
    r.call(scale, shift, res, True, x=x, cons=cons, no_float=True)  # NO_FLOAT: out is not written
    assert bool((r.out == 7.0).all()) and torch.equal(r.oq.cpu(), _twin(cons, want))
    r.call(scale, shift, res, True, x=x)  # no codes at all: cimq_module_forward_epilogue
    assert torch.equal(r.out, want)
