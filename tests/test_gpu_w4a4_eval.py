"""GPU: forward-only w4a4 layers in 1-bit slices on the stateless word-pair forward -- cim_fwd_v3_kernel<4, KS, 4, NONE,
INFER / EPI / CODES / VIEW, 1 / 2>, one launch per prepared layer, the activation quantised in the kernel's row staging
(fp32 x) or read as code bytes.

The reference of every equality is the training forward of the same layer on the same parameters: it quantises x in
prep_module_kernel (another code path than the staging), runs the word pairs with their state, and is itself held to
the module oracle by test_gpu_w4a4.py.  Every case asserts its form, cimq_module_forward_form == (4, 1), before it
launches: on a library without the form the symbol is missing and the case stops there.  No shape is gated back to the
per-k form (all six ResNet-20 shapes keep the new form), so no case expects (0, 0) and the launch
count of the one-call network is 18 single launches, the w8a8 first conv's two and the head: 21.

Bars: torch.equal (bit patterns where a NaN may occur) for every forward-only mode against the training forward or
the four torch operations on it; the module oracle's own bar for out (1e-6 of max(|ref|, sum of |terms|)); the head
bars of test_gpu_net.py for the logits.  Shapes: w4a4_cases.py at B = 2.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from conftest import REPO, rel_err
from oracle import cim_oracle as co
from test_gpu_codes import _ready, _twin
from test_gpu_epilogue import _fused, _plain, _ref, _tables
from test_gpu_fullsize import _capture_oracle_ctx, _oracle_codes
from test_gpu_net import _Plan, _bits, _head_bars, _logit_bar, _loop_last_plane
from test_gpu_rect import _module_data, _modules
from w4a4_cases import ADC_CASES, LITERAL_CASE, MODULE_CASES, case_id

pytestmark = pytest.mark.gpu

KW4 = dict(nbits_w=4, nbits_a=4, nbits_alpha=8, wbitslice=1, abitslice=1, xbar=128, adcbits=1.5, signed_xbar=True,
           stochastic_quant=False)
QP = 15


def _F():
    from cim_quantization_amd import functional as F
    return F


def _L():
    import cim_quantization_amd._lib as L
    return L


def _assert_form(m, x_shape, want=(4, 1)):
    """the form of the forward-only descriptor the module itself makes for this input"""
    F, L = _F(), _L()
    desc = F.module_descs(m, tuple(x_shape), inference=True)[0]
    assert (desc.bits_w, desc.bits_a, desc.bs_w, desc.bs_a) == (4, 4, 1, 1)
    assert desc.options & L.CIMQ_OPT_INFERENCE
    assert L.module_forward_form(desc) == want
    assert tuple(L.ROUTE_NAMES[v] for v in L.module_route(desc)) == ("v3", "none", "none")


def _train_out(m, x):
    """the training forward (prologue quantiser, word pairs with their state)"""
    m.train()
    return m(x.clone().requires_grad_(True)).detach()


def _unprepared(m, x):
    """the forward-only call with wprep NULL: the whole prologue's weight side in the call itself"""
    F = _F()
    with torch.no_grad():
        return F.cim_module_conv(x, m.weight, m.alpha_act, m.alpha_weight, m.alpha_cim, m.binary_mask.to(x.device),
                                 m.signed_act, *m.layer_config(), False, False, None, None, m.recompute_psum)


def _oracle_sa(om, x_np):
    """the activation step size the oracle module computes for an input of this size (the value alone: the data
    do not enter it)"""
    om.train()
    om(torch.from_numpy(np.abs(x_np)))  # (grad mode on: the oracle keeps its intermediates' grads)
    return float(om.dbg["sa"].item())


def _case(c, seed, dev):
    d = _module_data(c, seed, step="quantile")
    m, om = _modules(c, d, dev)
    assert (m.nbits_w, m.nbits_a, m.wbitslice, m.abitslice) == (4, 4, 1, 1)
    return d, m, om


# ---------------------------------------------------------------------------------------------------
# 1. every module case: the no-grad forward against the training forward and the oracle
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(MODULE_CASES)), ids=[case_id(c) for c in MODULE_CASES])
def test_forward_equals_training_forward(cuda_device, monkeypatch, idx):
    c = MODULE_CASES[idx]
    d, m, om = _case(c, 9400 + idx, cuda_device)
    x = torch.from_numpy(d["x"]).to(cuda_device)
    _assert_form(m, x.shape)
    ref = _train_out(m, x)
    v = _plain(m, x)  # prepared: the kept inference weight side
    assert v.shape == ref.shape and v.is_contiguous()
    assert torch.equal(v, ref), float((v - ref).abs().max())
    # the module oracle's bar for out
    box = _capture_oracle_ctx(monkeypatch)
    oout = om(torch.from_numpy(d["x"])).detach()
    cc = box["c"]
    bm = om.binary_mask.numpy()
    terms = (np.abs(cc.adc.astype(np.float64)) * np.abs(bm.astype(np.float64))).sum(axis=(1, 2, 3))
    terms = terms.transpose(0, 2, 1).reshape(oout.shape)
    assert (cc.adc != 0).mean() > 0.05
    assert rel_err(v.cpu().numpy(), oout.numpy(), terms) < 1e-6
    # prepared and unprepared: equal bits; two runs on the same buffers: equal bits
    u = _unprepared(m, x)
    assert torch.equal(_bits(u), _bits(v))
    assert torch.equal(_bits(_plain(m, x)), _bits(v)) and torch.equal(_bits(_unprepared(m, x)), _bits(v))


# ---------------------------------------------------------------------------------------------------
# 2. the literal paths: a multi-bit ADC, the sign ADC, the flagged alpha_cim
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(ADC_CASES)), ids=[case_id(c) for c in ADC_CASES])
def test_other_adc_modes(cuda_device, idx):
    c = ADC_CASES[idx]
    d, m, _ = _case(c, 9440 + idx, cuda_device)
    x = torch.from_numpy(d["x"]).to(cuda_device)
    _assert_form(m, x.shape)
    ref = _train_out(m, x)
    v = _plain(m, x)
    assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0
    assert torch.equal(v, ref), float((v - ref).abs().max())
    assert torch.equal(_bits(_unprepared(m, x)), _bits(v))


def test_literal_flag(cuda_device):
    """all-equal alpha_cim: the alpha quantiser's scale is 0, the literal ADC runs and the output is NaN throughout
    (test_gpu_alpha_equal holds the training forward to the oracle's NaN pattern): the same bits"""
    c = LITERAL_CASE
    d, m, _ = _case(c, 9460, cuda_device)
    with torch.no_grad():
        m.alpha_cim.fill_(0.05)
    x = torch.from_numpy(d["x"]).to(cuda_device)
    _assert_form(m, x.shape)
    ref = _train_out(m, x)
    assert torch.isnan(ref).all()
    v = _plain(m, x)
    assert torch.equal(_bits(v), _bits(ref))
    assert torch.equal(_bits(_unprepared(m, x)), _bits(ref))


# ---------------------------------------------------------------------------------------------------
# 3. the staging quantiser's edge cases
# ---------------------------------------------------------------------------------------------------
def test_staging_edge_cases(cuda_device):
    c = MODULE_CASES[0]
    d, m, om = _case(c, 9470, cuda_device)
    sa = _oracle_sa(om, d["x"])
    x = d["x"].copy()
    flat = x.reshape(-1)
    rng = np.random.default_rng(9471)
    pick = rng.permutation(flat.size)
    n = flat.size // 32
    flat[pick[0 * n:1 * n]] = -np.abs(flat[pick[0 * n:1 * n]]) - np.float32(0.1)                 # negatives
    flat[pick[1 * n:2 * n]] = (rng.integers(0, QP, n) + 0.5).astype(np.float32) * np.float32(sa)  # exact .5 sa ties
    flat[pick[2 * n:3 * n]] = np.float32(QP) * np.float32(sa)                                    # at Qp sa
    flat[pick[3 * n:4 * n]] = np.float32(QP + 0.5) * np.float32(sa)                              # the tie at the clamp
    flat[pick[4 * n:5 * n]] = np.float32(QP * 3) * np.float32(sa)                                # above
    special = pick[5 * n:5 * n + 12]
    flat[special[0:4]] = np.nan
    flat[special[4:8]] = np.inf
    flat[special[8:12]] = -np.inf
    flat[[0, flat.size - 1]] = np.nan  # the first and the last element
    xt = torch.from_numpy(x).to(cuda_device)
    _assert_form(m, xt.shape)
    # coverage, on the oracle's values (the NaN elements, a handful, as zeros: its slicing is not NaN-safe)
    xz = np.where(np.isnan(x), np.float32(0), x).astype(np.float32)
    om.train()
    om(torch.from_numpy(xz).requires_grad_(True))
    dd = om.dbg
    codes = np.rint(dd["x_q"].detach().numpy() / dd["sa"].item())
    assert dd["sa"].item() == sa
    assert (codes == QP).mean() >= 0.01 and codes.min() == 0 and codes.max() == QP
    alpha_q = co.alpha_quantize(om.alpha_cim.detach().numpy(), 8)
    oc, _ = _oracle_codes(dd["x_q"].detach().numpy(), dd["w_q"].detach().numpy(), c["s"], c["p"], 4, c["xbar"], alpha_q,
                          dd["sw"].detach().numpy().reshape(1), dd["sa"].detach().numpy().reshape(1), 0.0)
    nz = (oc != 0).mean(axis=(0, 1, 4, 5))  # per (k, j)
    print("nonzero codes per slice pair %.3f .. %.3f, activations at Qp %.4f" % (nz.min(), nz.max(),
                                                                                 (codes == QP).mean()))
    assert nz.shape == (4, 4) and nz.min() >= 0.05 and nz.max() <= 0.95, nz
    ref = _train_out(m, xt)
    v = _plain(m, xt)
    assert torch.equal(_bits(v), _bits(ref)), float((v - ref).abs().max())
    assert torch.equal(_bits(_unprepared(m, xt)), _bits(ref))
    # the same input as codes (NaN: code 16) gives the same bits
    one, zero = torch.ones(c["O"], device=cuda_device), torch.zeros(c["O"], device=cuda_device)
    xq = m.act_codes(xt.cpu()).to(cuda_device)
    assert int(xq.max()) == QP + 1
    assert torch.equal(_bits(_fused(m, xq, one, zero)), _bits(_fused(m, xt, one, zero)))


# ---------------------------------------------------------------------------------------------------
# 4. forward_fused: the epilogue instances
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [0, 2, 4], ids=[case_id(MODULE_CASES[i]) for i in (0, 2, 4)])
def test_forward_fused(cuda_device, idx):
    c = MODULE_CASES[idx]
    d, m, _ = _case(c, 9400 + idx, cuda_device)
    x = torch.from_numpy(d["x"]).to(cuda_device)
    _assert_form(m, x.shape)
    ref = _train_out(m, x)
    v = _plain(m, x)
    assert torch.equal(v, ref)
    scale, shift, res = _tables(v, 570 + idx)
    for kw in (dict(), dict(relu=True), dict(residual=res), dict(residual=res, relu=True)):
        got = _fused(m, x, scale, shift, **kw)
        want = _ref(ref, scale, shift, **kw)
        assert got.shape == v.shape and torch.equal(got, want), (kw.keys(), float((got - want).abs().max()))
    frac = float((_ref(ref, scale, shift, res, True) == 0).float().mean())
    assert 0.05 < frac < 0.95, frac  # (ReLU does cut, and not everything)
    a = _fused(m, x, scale, shift, residual=res, relu=True)
    assert torch.equal(a, _fused(m, x, scale, shift, residual=res, relu=True))


# ---------------------------------------------------------------------------------------------------
# 5. codes in and out
# ---------------------------------------------------------------------------------------------------
def _mk4(dev, cin, cout, stride, x, seed):
    """a fresh w4a4 Conv2dLSQCiM cin -> cout (3 x 3, pad 1) after its first-step initialisation on input x"""
    import cim_quantization_amd._modules as my_nn
    torch.manual_seed(seed)
    m = my_nn.Conv2dLSQCiM(cin, cout, 3, stride, 1, bias=False, **KW4)
    torch.nn.init.kaiming_normal_(m.weight)
    m = m.to(dev).train()
    m(x)
    return m


def test_codes_in(cuda_device):
    """x_codes holding every code 0 .. 15, the NaN code 16 and one byte of 200 (it reads the NaN entry): the output of
    the call on an fp32 x with those codes"""
    c = MODULE_CASES[0]
    d, m, om = _case(c, 9400, cuda_device)
    x = torch.from_numpy(d["x"]).to(cuda_device)
    _assert_form(m, x.shape)
    assert _ready(m, x) == (True, True)
    sa = _oracle_sa(om, d["x"])
    g = torch.Generator().manual_seed(9480)
    xq = torch.randint(0, QP + 1, x.shape, generator=g, dtype=torch.uint8)
    flat = xq.view(-1)
    flat[:QP + 1] = torch.arange(QP + 1, dtype=torch.uint8)
    nan_at = torch.tensor([QP + 1, 100, flat.numel() // 2 + 3, flat.numel() - 1])
    flat[nan_at] = QP + 1
    xf = (xq.to(torch.float32) * np.float32(sa)).contiguous()
    xf.view(-1)[nan_at] = float("nan")
    assert torch.equal(m.act_codes(xf), xq)  # (the fp32 twin has those codes)
    flat[100] = 200
    xq, xf = xq.to(cuda_device), xf.to(cuda_device)
    assert set(xq.view(-1).tolist()) == set(range(QP + 2)) | {200}
    v = _plain(m, xf)
    scale, shift, res = _tables(torch.nan_to_num(v), 581)
    for e in (dict(), dict(residual=res, relu=True)):
        got, want = _fused(m, xq, scale, shift, **e), _fused(m, xf, scale, shift, **e)
        assert torch.equal(_bits(got), _bits(want)), e.keys()
    # and against the training forward of that fp32 x
    one, zero = torch.ones_like(scale), torch.zeros_like(shift)
    assert torch.equal(_bits(_fused(m, xq, one, zero)), _bits(_train_out(m, xf)))


def test_codes_out(cuda_device):
    """out_codes for a consumer with Qp 15, beside the float plane and alone (CIMQ_CODES_NO_FLOAT): the torch
    quantiser's codes of the float result"""
    c = MODULE_CASES[0]
    d, m, _ = _case(c, 9400, cuda_device)
    x = torch.from_numpy(d["x"]).to(cuda_device)
    _assert_form(m, x.shape)
    ref = _train_out(m, x)
    scale, shift, res = _tables(ref, 582)
    ep = dict(residual=res, relu=True)
    y = _fused(m, x, scale, shift, **ep)
    assert torch.equal(y, _ref(ref, scale, shift, **ep))
    cons = _mk4(cuda_device, c["O"], 16, 1, y, 583)
    pos = y[y > 0].float().cpu()
    with torch.no_grad():
        cons.alpha_act.fill_(float(torch.quantile(pos[:1_000_000], 0.92)) / (QP - 0.5))
    _assert_form(cons, y.shape)
    want = _twin(cons, y)
    assert set(want.view(-1).tolist()) == set(range(QP + 1)) and float((want == QP).float().mean()) >= 0.01
    yf, q = _fused(m, x, scale, shift, out_quant=cons, **ep)
    assert q.dtype == torch.uint8 and q.shape == y.shape and torch.equal(yf, y)
    assert torch.equal(q.cpu(), want)
    q2 = _fused(m, x, scale, shift, out_quant=cons, keep_float=False, **ep)
    assert torch.is_tensor(q2) and torch.equal(q2.cpu(), want)
    # the consumer reads them: the output it gives on the fp32 plane
    s2, t2, r2 = _tables(_plain(cons, y), 584)
    assert torch.equal(_fused(cons, q, s2, t2, residual=r2, relu=True), _fused(cons, y, s2, t2, residual=r2, relu=True))


# ---------------------------------------------------------------------------------------------------
# 6. the residual as a view
# ---------------------------------------------------------------------------------------------------
def test_residual_view(cuda_device):
    """test_gpu_net's three-layer block at w4a4: a layer that writes the view's source (16 -> 16 at 16 x 16), the
    stride-2 case's shape (16 -> 32) that writes the case layer's input, and the case layer (32 -> 32 at 8 x 8), whose
    residual is the view src[:, :, ::2, ::2] on channels 8 .. 23"""
    dev = cuda_device
    c0, s, Cr, O = 8, 2, 16, 32
    st = MODULE_CASES[2]
    assert (st["C"], st["O"], st["H"], st["s"]) == (16, 32, 16, (2, 2))
    x0 = torch.randn(2, 16, 16, 16, generator=torch.Generator().manual_seed(9490)).relu().to(dev)
    p1 = _mk4(dev, 16, Cr, 1, x0, 9491)
    sa, ta, _ = _tables(_plain(p1, x0), 9492)
    y0 = _fused(p1, x0, sa, ta, relu=True)
    p2 = _mk4(dev, Cr, 32, s, y0, 9493)
    sb, tb, _ = _tables(_plain(p2, y0), 9494)
    y1 = _fused(p2, y0, sb, tb, relu=True)
    assert tuple(y1.shape) == (2, 32, 8, 8)
    m = _mk4(dev, 32, O, 1, y1, 9495)
    for mod, t in ((p1, x0), (p2, y0), (m, y1)):
        _assert_form(mod, t.shape)
    v = _plain(m, y1)
    assert torch.equal(v, _train_out(m, y1))
    sc, tc, _ = _tables(v, 9496)
    zs = [o for o in range(O - 1, -1, -1) if not (c0 <= o < c0 + Cr)]
    z = next((o for o in zs if bool((v[:, o] < 0).any())), zs[0])
    sc[z], tc[z] = 0.0, -0.0
    pad = TF.pad(y0[:, :, ::s, ::s], (0, 0, 0, 0, c0, O - c0 - Cr))
    assert tuple(pad.shape) == tuple(v.shape)
    for relu in (True, False):
        want = _fused(m, y1, sc, tc, residual=pad, relu=relu)
        bare = _fused(m, y1, sc, tc, relu=relu)
        assert bool((_bits(bare[:, z]) == -2 ** 31).any()) and bool((_bits(want[:, z]) == 0).all())
        try:
            for mod in (p1, p2, m):
                mod.eval()
            p = _Plan(x0)
            a, b, cs = p.slot(y0.shape), p.slot(y1.shape), p.slot(want.shape)
            p.layer(p1, x0.shape, sa, ta, True, -1, a)
            p.layer(p2, y0.shape, sb, tb, True, a, b)
            p.layer(m, y1.shape, sc, tc, relu, b, cs, res_slot=a, res_c0=c0, res_stride=s)
            L = _L()
            for it in p.items:
                assert L.module_forward_form(it["desc"]) == (4, 1)
            p.run()
            first = p.sf[cs].clone()
            p.run()
        finally:
            for mod in (p1, p2, m):
                mod.train()
        assert torch.equal(_bits(p.sf[a]), _bits(y0)) and torch.equal(_bits(p.sf[b]), _bits(y1))
        assert torch.equal(_bits(p.sf[cs]), _bits(want)), (relu, float((p.sf[cs] - want).abs().max()))
        assert torch.equal(_bits(first), _bits(p.sf[cs]))


# ---------------------------------------------------------------------------------------------------
# 7. / 8. the one-call network and validate
# ---------------------------------------------------------------------------------------------------
_NET4 = {}


def _tool():
    if "tool" not in _NET4:
        spec = importlib.util.spec_from_file_location("infer_net_bench", os.path.join(REPO, "tools", "infer_net_bench.py"))
        tool = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tool)
        _NET4["tool"] = tool
    return _NET4["tool"]


def _net4(dev):
    """tools/infer_net_bench.build_model(bits=4): ResNet-20, w4a4 (first conv w8a8), xbar 128, adc 1.5, at B = 2; the
    alpha_cim of every w4a4 conv then spread by 0.7 .. 1.3 as the module cases' is (the data-driven initial values
    are so regular that the 16 pairs' sum does not depend on its order)"""
    if "m" not in _NET4:
        model, x = _tool().build_model(2, dev, bits=4)
        g = torch.Generator().manual_seed(22)
        with torch.no_grad():
            for cv in _convs4(model):
                cv.alpha_cim.mul_((0.7 + 0.6 * torch.rand(cv.alpha_cim.shape, generator=g)).to(dev))
        _NET4["m"], _NET4["x"] = model, x
    return _NET4["m"], _NET4["x"]


def _convs4(model):
    from cim_quantization_amd._modules.lsq import Conv2dLSQCiM
    return [m for m in model.modules() if isinstance(m, Conv2dLSQCiM) and m.nbits_w == 4]


def test_fused_eval_net_w4a4(cuda_device):
    from cim_quantization_amd.harness.fuse import FusedEval
    model, x = _net4(cuda_device)
    convs = _convs4(model)
    assert len(convs) == 18
    sizes = {16: 32, 32: 16, 64: 8}
    for cv in convs:
        h = sizes[cv.in_channels]
        _assert_form(cv, (2, cv.in_channels, h, h))
    lin = model.linear
    with torch.no_grad():
        # the network's own forward on the forward-only calls and on the training forward's kernels (the switch
        # the suite has for this): every w4a4 conv's output plane and the logits, bit for bit
        F = _F()
        seen = {True: [], False: []}
        hooks = [cv.register_forward_hook(lambda mod, inp, out: seen[F._INFERENCE].append(out.clone())) for cv in convs]
        try:
            ya = model(x)
            F._INFERENCE = False
            yt = model(x)
        finally:
            F._INFERENCE = True
            for h in hooks:
                h.remove()
        assert len(seen[True]) == len(seen[False]) == 18
        for i, (pa, pt) in enumerate(zip(seen[True], seen[False])):
            assert torch.equal(_bits(pa), _bits(pt)), (i, float((pa - pt).abs().max()))
        assert torch.isfinite(ya).all() and torch.equal(_bits(ya), _bits(yt)), float((ya - yt).abs().max())
        plane, loop_logits = _loop_last_plane(model, x)
        fused = FusedEval(model, net=True)
        got = fused(x)
        assert fused.net_used is True, fused.net_reason
        last = fused._net_plan.last_plane().clone()
        assert torch.equal(_bits(last), _bits(plane))
        pooled = TF.avg_pool2d(last, last.shape[3]).flatten(1)
        pbar, lbar = _head_bars(last, pooled, lin.weight.detach(), lin.bias.detach())
        mean64 = last.double().cpu().mean(dim=(2, 3))
        want = mean64 @ lin.weight.detach().double().cpu().t() + lin.bias.detach().double().cpu()
        extra = (lin.weight.detach().double().cpu().abs().unsqueeze(0) * pbar.unsqueeze(1)).sum(dim=2)
        err = (got.double().cpu() - want).abs()
        print("w4a4 net logits: max error %.3e, bar %.3e" % (float(err.max()), float((lbar + extra).max())))
        assert bool((err <= lbar + extra).all())
        assert torch.equal(fused(x), got)
        fc = FusedEval(model, net=True, codes=True)
        gotc = fc(x)
        assert fc.net_used is True, fc.net_reason
        assert torch.equal(_bits(gotc), _bits(got))
        assert torch.equal(_bits(fc._net_plan.last_plane()), _bits(plane))


def test_fused_eval_net_launches_w4a4(cuda_device):
    """one forward's device kernels: 18 single launches, the w8a8 first conv's two and the head"""
    from cim_quantization_amd.harness.fuse import FusedEval
    tool = _tool()
    model, x = _net4(cuda_device)
    with torch.no_grad():
        loop, net = FusedEval(model), FusedEval(model, net=True)
        loop(x)
        net(x)
        n_loop = tool.count_launches(lambda: loop(x))
        n_net = tool.count_launches(lambda: net(x))
    assert net.net_used
    assert "error" not in n_loop and "error" not in n_net, (n_loop, n_net)
    print("w4a4 device kernels per forward: loop %s, net %s" % (n_loop, n_net))
    assert n_net["kernels"] == n_net["libcimq"] == 21
    assert n_net["libcimq"] == n_loop["libcimq"] + 1


def test_validate_net_w4a4(cuda_device):
    from cim_quantization_amd.harness import train
    model, x = _net4(cuda_device)
    g = torch.Generator().manual_seed(6)
    batches = [(torch.randn(2, 3, 32, 32, generator=g).to(cuda_device),
                torch.randint(0, 10, (2,), generator=g).to(cuda_device)) for _ in range(2)]

    class HP:
        overfit_test = False

    crit = torch.nn.CrossEntropyLoss()
    got = train.validate(batches, model, crit, HP, fused=True, net=True)
    want = train.validate(batches, model, crit, HP, fused=True)
    with torch.no_grad():
        bar = max(_logit_bar(_loop_last_plane(model, bx)[0], model) for bx, _ in batches)
    print("w4a4 validate: loss %.9g (net) vs %.9g (loop), bound %.3e" % (got[2], want[2], 2 * bar))
    assert abs(got[2] - want[2]) <= 2 * bar
