"""GPU parity on rectangular images (H != W) and anisotropic kernels / strides / paddings, on every kernel route.

Every other GPU test builds (B, C, H, H) inputs with k x k kernels and one stride and padding for both axes, yet the
plans (cimq_host.h) gate the fast kernels on W, Wo, P and M and leave H almost free, so rectangular layers take the
fast routes.  The shapes here reach what square power-of-two shapes cannot: image rows against image columns, m-tiles
per image that are no power of two, whole-image m-tiles (P < 128), the fused kernel with R = 64 / W != H, a partial
last grad_x band, and W = 64 (the widest the plans admit) on 4 x 64 and 16 x 64 images.  The cases and the route each
must take are rect_cases.py's (test_rect_routes_host.py asserts the routes on the CPU too).

Bars, the suite's own: integer partial sums and ADC outputs bit-exact; out within 1e-6 and the gradients within 1e-5 of
max(|ref|, sum of |terms|) element by element; ADC codes and STE-pass bits of the state words equal to the oracle's;
the forward-only modes torch.equal.  General-route cases run first in every table.
"""
import math

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import cim_module_oracle as cmo
from oracle import cim_oracle as co
from rect_cases import (BAND_CASE, FORWARD_ONLY, FUNCTION_CASES, MODULE_CASES, SHIFT_CASES, case_id, make_desc, out_hw,
                        route_names)
from test_gpu_epilogue import _fused, _plain, _ref, _tables
from test_gpu_fullsize import _capture_oracle_ctx, _check_elementwise, _kw, _lsq_scalar_terms, _oracle_codes, _pin
from test_gpu_parity import _check_integer_steps, _random_inputs, _sampled_images_and_properties, run_hip_function

pytestmark = pytest.mark.gpu


def _L():
    import cim_quantization_amd._lib as L
    return L


# ------------------------------------------------------------------------------------------
# the Function path
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(FUNCTION_CASES)), ids=[case_id(c) for c in FUNCTION_CASES])
def test_function_vs_oracle_rect(cuda_device, idx):
    """get_cim_output_signed on [B, P, O] against cim_forward / cim_backward, asserted as
    test_gpu_parity.test_function_vs_oracle_random does"""
    cfg = FUNCTION_CASES[idx]
    inp = _random_inputs(cfg, 7300 + idx)
    st, pd = cfg["s"], cfg["p"]
    out, c = co.cim_forward(inp["x_q"], inp["w_q"], st, pd, (1, 1), cfg["ab"], cfg["abs"], cfg["wb"], cfg["wbs"],
                            cfg["adc"], cfg["xbar"], inp["binary_mask"], inp["alpha_q"], inp["sw"], inp["sa"],
                            False, inp["signed_act"], return_debug=True)
    ho, wo = out_hw(cfg)
    assert out.shape == (cfg["B"], ho * wo, cfg["O"])
    gx, gw, ga = co.cim_backward(c, inp["grad"])
    ax, aw, aa = co.cim_backward(c, inp["grad"], absolute=True)
    res = run_hip_function(cuda_device, cfg, inp)
    _check_integer_steps(cfg, inp, res, c.ps16)
    out_terms = np.sum(np.abs(c.adc.astype(np.float64) * inp["binary_mask"]), axis=(1, 2, 3))
    assert res["out"].shape == out.shape and res["grad_x"].shape == gx.shape and res["grad_w"].shape == gw.shape
    assert rel_err(res["out"], out, out_terms) < 1e-6
    assert rel_err(res["grad_x"], gx, ax) < 1e-5
    assert rel_err(res["grad_w"], gw, aw) < 1e-5
    if ga is not None:
        assert rel_err(res["grad_alpha"], ga, aa) < 1e-5


# ------------------------------------------------------------------------------------------
# the module path, steady state
# ------------------------------------------------------------------------------------------
def _module_data(c, seed, step="mean"):
    """weights, input, output gradient and the pinned state of a case: the step sizes of lsq.py:539-542 on the
    data (``step`` "quantile": the 97 % points of x and |w| over Qp instead, so that a few per cent of the values
    clamp and the top slices of wide codes are filled), a data-driven alpha_cim (lsq.py:557-563) at the case's bit
    and slice widths, spread so that the codes vary"""
    rng = np.random.default_rng(seed)
    B, C, O, H, W = c["B"], c["C"], c["O"], c["H"], c["W"]
    k = (c["kh"], c["kw"])
    w = (rng.standard_normal((O, C) + k) * math.sqrt(2.0 / (k[0] * k[1] * C))).astype(np.float32)
    x = rng.standard_normal((B, C, H, W)).astype(np.float32)
    if not c["signed"]:
        x = np.maximum(x, 0)
    ho, wo = out_hw(c)
    g = (rng.standard_normal((B, O, ho, wo)) / math.sqrt(B * O * ho * wo)).astype(np.float32)
    qp_a, (qn_w, qp_w) = 2 ** c["ab"] - 1, co.lsq_weight_params(c["wb"])
    if step == "quantile":
        aa = np.float32(np.quantile(x, 0.97) / qp_a)
        aw = np.float32(np.quantile(np.abs(w), 0.97) / qp_w)
    else:
        aa = np.float32(2 * np.abs(x).mean() / math.sqrt(qp_a))
        aw = np.float32(2 * np.abs(w).mean() / math.sqrt(qp_w))
    ac = None
    if c["adc"] in (1, 1.5):
        sa0 = co.grad_scale_value(np.array([aa], np.float32), 1.0 / math.sqrt(x.size * qp_a))
        sw0 = co.grad_scale_value(np.array([aw], np.float32), 1.0 / math.sqrt(w.size * qp_w))
        xq0, _ = co.lsq_quantize(x, sa0, 0, qp_a)
        wq0, _ = co.lsq_quantize(w, sw0, qn_w, qp_w)
        ac = co.alpha_cim_init(xq0, wq0, c["s"], c["p"], c["ab"], c["abs"], c["wb"], c["wbs"], c["xbar"], sw0, sa0,
                               c["adc"])
        ac = (ac * (0.7 + 0.6 * rng.random(ac.shape))).astype(np.float32)
    return dict(x=x, w=w, g=g, aa=aa, aw=aw, ac=ac, qp_a=qp_a, qn_w=qn_w, qp_w=qp_w)


def _modules(c, d, dev, oracle=True):
    import cim_quantization_amd._modules as my_nn
    k = (c["kh"], c["kw"])
    kw = _kw(c["wb"], c["xbar"], c["adc"], c["ab"], c["wbs"], c["abs"])
    m = my_nn.Conv2dLSQCiM(c["C"], c["O"], k, c["s"], c["p"], bias=False, **kw).to(dev)
    m.recompute_psum = c["recompute"]
    mods = [m]
    if oracle:
        om = cmo.OracleConv2dLSQCiM(c["C"], c["O"], k, c["s"], c["p"], (1, 1), bias=False, **kw)
        om.debug_retain = True
        mods.append(om)
    for mod in mods:
        with torch.no_grad():
            mod.weight.copy_(torch.from_numpy(d["w"]))
    _pin(mods, d["aa"], d["aw"], d["ac"])
    if c["signed"]:
        for mod in mods:
            mod.signed_act.fill_(1)
            mod._state_cache = None
    return mods


def _assert_route(c, m, x_shape):
    """the route of the descriptor the module itself makes for this input, and of the table's descriptor"""
    from cim_quantization_amd import functional as F
    L = _L()
    want = c["route"]
    assert route_names(L, make_desc(L, c)) == want
    assert route_names(L, F.module_descs(m, tuple(x_shape))[0]) == want


@pytest.mark.parametrize("idx", range(len(MODULE_CASES)), ids=[case_id(c) for c in MODULE_CASES])
def test_module_vs_oracle_rect(cuda_device, monkeypatch, idx):
    """Conv2dLSQCiM in steady state against the module oracle on the whole batch, asserted as
    test_gpu_fullsize.test_resnet20_layer_module_fullbatch does, on the route the case names"""
    from cim_quantization_amd import functional as F
    c = MODULE_CASES[idx]
    d = _module_data(c, 8300 + idx)
    m, om = _modules(c, d, cuda_device)
    x, w, g = d["x"], d["w"], d["g"]
    _assert_route(c, m, x.shape)
    ho, wo = out_hw(c)

    xt = torch.from_numpy(x).to(cuda_device).requires_grad_(True)
    out = m(xt)
    assert tuple(out.shape) == (c["B"], c["O"], ho, wo) and out.is_contiguous()
    # the state words exist where the backward reads compact v7 words (or recomputes them: r6's debug path); they hold
    # the ternary ADC's code and pass bit
    has_codes = c["adc"] == 1.5 and c["route"][1] in ("v7", "gx5", "fused", "r6")
    code, passed = F.debug_state_codes(out) if has_codes else (None, None)
    out.backward(torch.from_numpy(g).to(cuda_device))
    torch.cuda.synchronize()

    box = _capture_oracle_ctx(monkeypatch)
    ox = torch.from_numpy(x).requires_grad_(True)
    oout = om(ox)
    assert tuple(oout.shape) == tuple(out.shape)
    oout.backward(torch.from_numpy(g))
    cc = box["c"]

    if m.alpha_cim is not None:
        _check_elementwise(cc, om.binary_mask.numpy(), g, out, oout, xt, ox, m, om)
    else:
        g_bpo = np.ascontiguousarray(g.reshape(c["B"], c["O"], -1).transpose(0, 2, 1))
        ax, aw, _ = co.cim_backward(cc, g_bpo, absolute=True)
        np_ = lambda t: t.detach().cpu().numpy()  # noqa: E731
        bm = np.abs(om.binary_mask.numpy().astype(np.float64))
        out_terms = (np.abs(cc.adc.astype(np.float64)) * bm).sum(axis=(1, 2, 3)).transpose(0, 2, 1)
        assert rel_err(np_(out), np_(oout), out_terms.reshape(np_(oout).shape)) < 1e-6, "out"
        assert rel_err(np_(xt.grad), np_(ox.grad), ax.reshape(x.shape)) < 1e-5, "grad_x"
        assert rel_err(np_(m.weight.grad), np_(om.weight.grad), aw.reshape(w.shape)) < 1e-5, "grad_w"
    dd = om.dbg
    t_act = _lsq_scalar_terms(x, dd["x_q"].grad.numpy(), dd["sa"].item(), 0, d["qp_a"],
                              1.0 / math.sqrt(x.size * d["qp_a"]))
    t_w = _lsq_scalar_terms(w, dd["w_q"].grad.numpy(), dd["sw"].item(), d["qn_w"], d["qp_w"],
                            1.0 / math.sqrt(w.size * d["qp_w"]))
    assert abs(m.alpha_act.grad.item() - om.alpha_act.grad.item()) <= 1e-5 * t_act
    assert abs(m.alpha_weight.grad.item() - om.alpha_weight.grad.item()) <= 1e-5 * t_w

    if not has_codes:
        return
    bits = c["wb"]
    alpha_q = co.alpha_quantize(om.alpha_cim.detach().numpy(), 8)
    sw_np, sa_np = dd["sw"].detach().numpy().reshape(1), dd["sa"].detach().numpy().reshape(1)
    oc, op = _oracle_codes(dd["x_q"].detach().numpy(), dd["w_q"].detach().numpy(), c["s"], c["p"], bits, c["xbar"],
                           alpha_q, sw_np, sa_np, float(c["signed"]))
    mc, mp = code.cpu().numpy(), passed.cpu().numpy()
    assert mc.shape == oc.shape
    assert np.array_equal(mc, oc), f"ADC codes differ at {np.argwhere(mc != oc)[:5].tolist()}"
    assert np.array_equal(mp, op), f"STE pass bits differ at {np.argwhere(mp != op)[:5].tolist()}"
    assert (oc != 0).mean() > 0.05 and (oc == 0).mean() > 0.05, "codes must vary for the check to bite"


# ------------------------------------------------------------------------------------------
# a partial last grad_x band
# ------------------------------------------------------------------------------------------
def test_partial_grad_x_band(cuda_device):
    """B = 128, 32 -> 32, 12 x 32, stride 1.  v7_plan takes rb = 8 at stride 1 and halves it only while
    B * ceil(H / rb) < 256; here 128 * ceil(12 / 8) = 256, so RB = min(H, 8) = 8 and nbands = ceil(12 / 8) = 2: an
    8-row band and a partial 4-row one, which no square power-of-two image has.  The full-batch oracle would hold
    some 40 M partial sums in several fp64 copies, so: determinism, linearity of the backward in grad_out on the whole
    batch, and out / grad_x / the integer partial sums of images 0 and B - 1 against the oracle."""
    L = _L()
    c = BAND_CASE
    assert route_names(L, make_desc(L, c)) == c["route"]
    assert c["B"] * math.ceil(c["H"] / 8) >= 256 and c["H"] % 8 == 4
    _sampled_images_and_properties(cuda_device, c, 9150)


# ------------------------------------------------------------------------------------------
# the forward-only modes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", FORWARD_ONLY, ids=[case_id(MODULE_CASES[i]) for i in FORWARD_ONLY])
def test_forward_only_modes_rect(cuda_device, idx):
    c = MODULE_CASES[idx]
    d = _module_data(c, 8300 + idx)
    m, = _modules(c, d, cuda_device, oracle=False)
    _assert_route(c, m, d["x"].shape)
    x = torch.from_numpy(d["x"]).to(cuda_device)
    train_out = m(x.clone().requires_grad_(True)).detach()
    v = _plain(m, x)
    ho, wo = out_hw(c)
    assert tuple(v.shape) == (c["B"], c["O"], ho, wo)
    assert torch.equal(v, train_out), float((v - train_out).abs().max())
    scale, shift, res = _tables(v, 400 + idx)
    assert tuple(res.shape) == (c["B"], c["O"], ho, wo)
    got = _fused(m, x, scale, shift, residual=res, relu=True)
    want = _ref(v, scale, shift, res, True)
    assert got.shape == v.shape and torch.equal(got, want), float((got - want).abs().max())
    frac = float((want == 0).float().mean())
    assert 0.05 < frac < 0.95, frac  # (ReLU does cut, and not everything)


# ------------------------------------------------------------------------------------------
# the shift ADC module
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SHIFT_CASES, ids=case_id)
def test_shift_module_vs_oracle_rect(cuda_device, monkeypatch, c):
    """Conv2dLSQCiM(adc_shift=True) on libcimq's fused shift path, with test_gpu_shift_fullbatch's assertions
    (grad_beta and run-to-run bit identity included)"""
    from cim_quantization_amd import functional as F
    from test_gpu_shift_fullbatch import _check
    L = _L()
    d = make_desc(L, c, variant=L.CIMQ_ADC_SHIFT_ROUND)
    assert route_names(L, d) == c["route"]
    m = _check(cuda_device, monkeypatch, c["C"], c["O"], c["H"], 1, c["wb"], c["B"], 9500 + c["W"], signed=False,
               W=c["W"], xbar=c["xbar"])
    assert m._shift_fused(torch.empty(c["B"], c["C"], c["H"], c["W"], device=cuda_device))
    desc, _ = F._shift_module_descs((c["B"], c["C"], c["H"], c["W"]), m.weight, m.stride, m.padding, m.dilation,
                                    m.nbits_a, m.abitslice, m.nbits_w, m.wbitslice, m.xbar, m.nbits_alpha)
    assert route_names(L, desc) == c["route"]


# ------------------------------------------------------------------------------------------
# the first step on a rectangular input
# ------------------------------------------------------------------------------------------
def test_first_step_rect(cuda_device):
    """A fresh layer in training mode on a (2, 16, 8, 32) input: the first step (sign detection, step sizes and
    alpha_cim from the data; torch quantisers around the CiM Function) returns (B, O, Ho, Wo), leaves alpha_cim as the
    oracle's lsq.py:557-563 on the same step sizes, and the next, steady-state step matches ``fused = False``."""
    from test_gpu_module_fused import _build, _grads, _step_size_terms
    cfg = dict(B=2, C=16, O=16, H=8, s=1, wb=3, ab=3, adc=1.5, xbar=128, bias=False)
    gen = torch.Generator().manual_seed(31)
    xs = [torch.randn(2, 16, 8, 32, generator=gen).relu().to(cuda_device) for _ in range(2)]
    ref = _build(cfg, cuda_device, 77)
    fus = _build(cfg, cuda_device, 77)
    fus.load_state_dict(ref.state_dict())
    ref.fused = False
    for m in (ref, fus):
        y = m(xs[0].clone().requires_grad_(True))
        assert tuple(y.shape) == (2, 16, 8, 32)
        y.backward(torch.ones_like(y))
        assert m.init_state.item() == 1 and m.init_state_cim.item() == 1 and m.signed_act.item() == 0
        for p in m.parameters():
            p.grad = None
    # alpha_cim on the step sizes the module found (test_gpu_parity.test_module_init_vs_golden's comparison)
    x0, w = xs[0].cpu().numpy(), fus.weight.detach().cpu().numpy()
    qp_a, (qn_w, qp_w) = 7, co.lsq_weight_params(3)
    sa = co.grad_scale_value(fus.alpha_act.detach().cpu().numpy(), 1.0 / math.sqrt(x0.size * qp_a))
    sw = co.grad_scale_value(fus.alpha_weight.detach().cpu().numpy(), 1.0 / math.sqrt(w.size * qp_w))
    xq, _ = co.lsq_quantize(x0, sa, 0, qp_a)
    wq, _ = co.lsq_quantize(w, sw, qn_w, qp_w)
    a0 = co.alpha_cim_init(xq, wq, (1, 1), (1, 1), 3, 1, 3, 1, 128, sw, sa, 1.5)
    assert rel_err(fus.alpha_cim.detach().cpu().numpy(), a0) < 1e-5
    # the steady state from one shared state (test_gpu_module_fused.test_fused_module_matches_torch_quantisers)
    fus.load_state_dict(ref.state_dict())
    x = xs[1]
    outs, grads, gxs = [], [], []
    for m in (ref, fus):
        xi = x.clone().requires_grad_(True)
        y = m(xi)
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(8)).to(cuda_device)
        y.backward(gy)
        outs.append(y.detach())
        gxs.append(xi.grad.detach())
        grads.append(_grads(m))
    tol = lambda a: 1e-5 * max(float(a.abs().max()), 1e-30)  # noqa: E731
    assert outs[0].shape == outs[1].shape == (2, 16, 8, 32)
    assert (outs[0] - outs[1]).abs().max() <= tol(outs[0]), "out"
    assert (gxs[0] - gxs[1]).abs().max() <= tol(gxs[0]) + 1e-12, "grad_x"
    t_terms = _step_size_terms(cfg, ref, x, gy)
    for name in grads[0]:
        a, b = grads[0][name], grads[1][name]
        if a.numel() == 1:
            assert abs(float(a) - float(b)) <= 1e-5 * t_terms[name], name
        else:
            assert (a - b).abs().max() <= tol(a) + 1e-12, name
