"""GPU parity with weight and activation slices wider than one bit (wbitslice / abitslice != 1) on every kernel route.

The plans (cimq_host.h) do not keep such layers off the fast kernels, yet every other GPU test but two small
general-route Function cases runs 1-bit slices.  What depends on the slice width there: the digit extraction of the
activation and weight words (a runtime shift and mask per slice), the code -> word tables of the code-reading
prologue, the 2^-(bs * j) and 2^-(bs * k) factors of grad_x and grad_w (as exponents of ldexpf, or as coefficients of
the params kernel), the search range of the ADC thresholds (+-psmax grows by 2^(bsa + bsw)) and the q tables of the
shift ADC.  The cases and the route each must take are slice_cases.py's (test_slice_routes_host.py asserts the routes
on the CPU too), and every case asserts its route before it launches.

Bars, the suite's own: integer partial sums and ADC outputs bit-exact; out within 1e-6 and the gradients within 1e-5 of
max(|ref|, sum of |terms|) element by element; ADC codes and STE-pass bits of the state words equal to the oracle's;
the forward-only modes torch.equal.  General-route cases run first in every table.
"""
import math

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import cim_oracle as co
from rect_cases import make_desc, out_hw, route_names
from slice_cases import (CODE_CASES, FORWARD_ONLY, FP16_CASE, FUNCTION_CASES, MODULE_CASES, SHIFT_CASES, case_id,
                         codes_expected)
from test_gpu_codes import _plant_nans, _ready, _twin
from test_gpu_epilogue import _fused, _plain, _ref, _tables
from test_gpu_fullsize import _capture_oracle_ctx, _check_elementwise, _kw, _lsq_scalar_terms, _oracle_codes
from test_gpu_parity import _check_integer_steps, _random_inputs, run_hip_function
from test_gpu_rect import _assert_route, _module_data, _modules

pytestmark = pytest.mark.gpu


def _L():
    import cim_quantization_amd._lib as L
    return L


# ------------------------------------------------------------------------------------------
# the Function path
# ------------------------------------------------------------------------------------------
def _ps_bound(cfg):
    """the largest |partial sum| of in-range digits over one crossbar tile"""
    K = cfg["C"] * cfg["kh"] * cfg["kw"]
    return min(K, cfg["xbar"]) * (2 ** cfg["abs"] - 1) * (2 ** cfg["wbs"] - 1)


def _exact_ps(c):
    """the integer partial sums: the product of the oracle's slices (rounded to the digits they stand for) per
    crossbar tile, in fp64 -- exact, where the reference's own sums pass through an fp16 store (lsq.py:169)"""
    xs, ws = np.rint(c.xs.astype(np.float64)), np.rint(c.ws.astype(np.float64))
    ps = np.empty(c.ps16.shape, np.float64)
    for i, (lo, hi) in enumerate(co._tiles(c.meta["K"], c.meta["arr"])):
        for j in range(c.meta["nba"]):
            for k in range(c.meta["nbw"]):
                ps[:, i, k, j] = np.matmul(xs[:, j, :, lo:hi], ws[k, lo:hi, :])
    assert np.abs(ps).max() < 2 ** 31
    return ps.astype(np.int64)


def _check_integer_steps_wide(cfg, inp, res, c):
    """_check_integer_steps for partial sums past 2048, where fp16 no longer holds every integer: debug_partial_sums
    returns the exact integer and the library's ADC reads its fp16 store (u_of), so ps is compared with the exact
    product of the slices -- and with round(reference ps), as _check_integer_steps does, wherever fp16 is exact -- and
    the ADC outputs with the reference ADC of fp16(ps)"""
    exact = _exact_ps(c)
    assert np.array_equal(res["ps"].astype(np.int64), exact), "integer partial sums differ"
    small = np.abs(exact) <= 2048
    assert np.array_equal(np.rint(c.ps16.astype(np.float64)).astype(np.int64)[small], exact[small])
    stored = exact.astype(np.float16)
    _, adc_ref = co.adc_apply(stored, cfg["adc"], inp.get("alpha_q"), inp["sw"], inp["sa"])
    mine = res["adc"]
    same = (mine == adc_ref) | (np.isnan(mine) & np.isnan(adc_ref))
    assert same.all(), f"ADC outputs differ at {np.argwhere(~same)[:5].tolist()}"
    # and the reference's own ADC (on its fp16 ps) agrees wherever its ps had no fp32 residue
    _, adc_ref16 = co.adc_apply(c.ps16, cfg["adc"], inp.get("alpha_q"), inp["sw"], inp["sa"])
    agree = c.ps16 == stored
    assert ((mine == adc_ref16) | np.isnan(adc_ref16) | ~agree).all()
    return exact


def _function_oracle(cfg, inp):
    out, c = co.cim_forward(inp["x_q"], inp["w_q"], cfg["s"], cfg["p"], (1, 1), cfg["ab"], cfg["abs"], cfg["wb"],
                            cfg["wbs"], cfg["adc"], cfg["xbar"], inp["binary_mask"], inp["alpha_q"], inp["sw"],
                            inp["sa"], False, inp["signed_act"], return_debug=True)
    return out, c


def _assert_function_floats(cfg, inp, res, out, c):
    gx, gw, ga = co.cim_backward(c, inp["grad"])
    ax, aw, aa = co.cim_backward(c, inp["grad"], absolute=True)
    out_terms = np.sum(np.abs(c.adc.astype(np.float64) * inp["binary_mask"]), axis=(1, 2, 3))
    assert res["out"].shape == out.shape and res["grad_x"].shape == gx.shape and res["grad_w"].shape == gw.shape
    assert rel_err(res["out"], out, out_terms) < 1e-6
    assert rel_err(res["grad_x"], gx, ax) < 1e-5
    assert rel_err(res["grad_w"], gw, aw) < 1e-5
    if ga is not None:
        assert rel_err(res["grad_alpha"], ga, aa) < 1e-5


@pytest.mark.parametrize("idx", range(len(FUNCTION_CASES)), ids=[case_id(c) for c in FUNCTION_CASES])
def test_function_vs_oracle_slices(cuda_device, idx):
    """get_cim_output_signed on [B, P, O] against cim_forward / cim_backward, asserted as
    test_gpu_parity.test_function_vs_oracle_random does"""
    cfg = FUNCTION_CASES[idx]
    inp = _random_inputs(cfg, 7600 + idx)
    assert inp["binary_mask"].shape[2:4] == (cfg["wb"] // cfg["wbs"], cfg["ab"] // cfg["abs"])
    out, c = _function_oracle(cfg, inp)
    ho, wo = out_hw(cfg)
    assert out.shape == (cfg["B"], ho * wo, cfg["O"])
    # every slice of either side is in use: the largest digit in each activation slice, and in each weight slice a
    # digit with its top bit set (the top slice of a signed b-bit code holds b - 1 magnitude bits, but for Qn)
    xtop = np.abs(np.rint(c.xs)).max(axis=(0, 2, 3))
    wtop = np.abs(np.rint(c.ws)).max(axis=(1, 2))
    assert (xtop >= 2 ** cfg["abs"] - 1).all() and (wtop >= 2 ** (cfg["wbs"] - 1)).all(), (xtop, wtop)
    res = run_hip_function(cuda_device, cfg, inp)
    if _ps_bound(cfg) <= 2048:
        _check_integer_steps(cfg, inp, res, c.ps16)
    else:
        _check_integer_steps_wide(cfg, inp, res, c)
    _assert_function_floats(cfg, inp, res, out, c)


def test_function_fp16_store_of_wide_sums(cuda_device):
    """4-bit slices on a 128-row tile reach |ps| > 2048, where the reference's fp16 store of the partial sums
    (lsq.py:169) rounds: 8 / 8 bits in 4-bit slices, C = 32 (every tile but the last has 128 rows), activations
    without the zeroing, power-of-two scales so that every slice is an exact integer.  The library's integer ps is
    the exact product of the slices, its ADC outputs are the reference ADC of the reference's fp16-rounded sums, and
    the case does reach sums that fp16 cannot hold."""
    cfg = FP16_CASE
    inp = _random_inputs(cfg, 7700)
    rng = np.random.default_rng(7701)
    codes = rng.integers(0, 2 ** cfg["ab"], size=inp["x_q"].shape).astype(np.float32)  # (no zeroing)
    inp["x_q"] = (codes * inp["sa"]).astype(np.float32)
    out, c = _function_oracle(cfg, inp)
    assert np.array_equal(c.xs, np.rint(c.xs)) and np.array_equal(c.ws, np.rint(c.ws))  # exact integer slices
    exact = _exact_ps(c)
    wide = (np.abs(exact) > 2048) & (exact.astype(np.float16).astype(np.int64) != exact)
    print(f"|ps| > 2048: {(np.abs(exact) > 2048).mean():.4f} of {exact.size}, max |ps| {np.abs(exact).max()}, "
          f"fp16(ps) != ps: {int(wide.sum())}")
    assert int(wide.sum()) >= 50
    # with integer slices the reference's fp32 sums are exact below 2^24, so its fp16 store is that of the integer
    assert np.array_equal(c.ps16, exact.astype(np.float16))
    res = run_hip_function(cuda_device, cfg, inp)
    assert np.array_equal(res["ps"].astype(np.int64), exact), "integer partial sums differ"
    _, adc_ref16 = co.adc_apply(c.ps16, cfg["adc"], inp["alpha_q"], inp["sw"], inp["sa"])
    assert np.array_equal(res["adc"], adc_ref16), f"ADC outputs differ at {np.argwhere(res['adc'] != adc_ref16)[:5]}"
    # the rounding matters: some of those sums change their ADC output with it
    _, adc_exact = co.adc_apply(exact.astype(np.float32), cfg["adc"], inp["alpha_q"], inp["sw"], inp["sa"])
    print(f"ADC outputs the fp16 store changes: {int((adc_exact != adc_ref16).sum())}")
    _assert_function_floats(cfg, inp, res, out, c)


# ------------------------------------------------------------------------------------------
# the module path, steady state
# ------------------------------------------------------------------------------------------
def _coverage(c, dd, d, oc):
    """the oracle's values must exercise what the widths add: every slice pair's ADC codes vary, activations reach
    Qp and weights both clamp ends (so the top slices and the clamps are in use)"""
    nz = (oc != 0).mean(axis=(0, 1, 4, 5))  # per (k, j)
    print(f"{case_id(c)}: nonzero codes per slice pair {np.round(nz, 3).tolist()}, max |ps| {d.get('psmax')}")
    assert nz.min() >= 0.05 and nz.max() <= 0.95, nz
    xr = np.rint(dd["x_q"].detach().numpy() / dd["sa"].item())
    wr = np.rint(dd["w_q"].detach().numpy() / dd["sw"].item())
    at_qp = (np.abs(xr) == d["qp_a"]).mean()
    print(f"activations at Qp {at_qp:.4f}, weights at Qn {(wr == d['qn_w']).mean():.4f}, at Qp "
          f"{(wr == d['qp_w']).mean():.4f}")
    assert at_qp >= 0.01
    assert (wr == d["qn_w"]).any() and (wr == d["qp_w"]).any()


@pytest.mark.parametrize("idx", range(len(MODULE_CASES)), ids=[case_id(c) for c in MODULE_CASES])
def test_module_vs_oracle_slices(cuda_device, monkeypatch, idx):
    """Conv2dLSQCiM in steady state against the module oracle on the whole batch, asserted as
    test_gpu_rect.test_module_vs_oracle_rect does, on the route the case names"""
    from cim_quantization_amd import functional as F
    c = MODULE_CASES[idx]
    d = _module_data(c, 8600 + idx, step="quantile")
    m, om = _modules(c, d, cuda_device)
    assert (m.wbitslice, m.abitslice, om.wbitslice, om.abitslice) == (c["wbs"], c["abs"], c["wbs"], c["abs"])
    x, w, g = d["x"], d["w"], d["g"]
    _assert_route(c, m, x.shape)
    ho, wo = out_hw(c)

    xt = torch.from_numpy(x).to(cuda_device).requires_grad_(True)
    out = m(xt)
    assert tuple(out.shape) == (c["B"], c["O"], ho, wo) and out.is_contiguous()
    # the state words exist where the backward reads compact v7 words; they hold the ternary ADC's code and pass bit
    has_codes = c["route"][1] in ("v7", "gx5", "fused")
    code, passed = F.debug_state_codes(out) if has_codes else (None, None)
    out.backward(torch.from_numpy(g).to(cuda_device))
    torch.cuda.synchronize()

    box = _capture_oracle_ctx(monkeypatch)
    ox = torch.from_numpy(x).requires_grad_(True)
    oout = om(ox)
    assert tuple(oout.shape) == tuple(out.shape)
    oout.backward(torch.from_numpy(g))
    cc = box["c"]

    _check_elementwise(cc, om.binary_mask.numpy(), g, out, oout, xt, ox, m, om)
    dd = om.dbg
    t_act = _lsq_scalar_terms(x, dd["x_q"].grad.numpy(), dd["sa"].item(), 0, d["qp_a"],
                              1.0 / math.sqrt(x.size * d["qp_a"]))
    t_w = _lsq_scalar_terms(w, dd["w_q"].grad.numpy(), dd["sw"].item(), d["qn_w"], d["qp_w"],
                            1.0 / math.sqrt(w.size * d["qp_w"]))
    assert abs(m.alpha_act.grad.item() - om.alpha_act.grad.item()) <= 1e-5 * t_act
    assert abs(m.alpha_weight.grad.item() - om.alpha_weight.grad.item()) <= 1e-5 * t_w

    alpha_q = co.alpha_quantize(om.alpha_cim.detach().numpy(), 8)
    sw_np, sa_np = dd["sw"].detach().numpy().reshape(1), dd["sa"].detach().numpy().reshape(1)
    oc, op = _oracle_codes(dd["x_q"].detach().numpy(), dd["w_q"].detach().numpy(), c["s"], c["p"], c["wb"], c["xbar"],
                           alpha_q, sw_np, sa_np, float(c["signed"]), c["ab"], c["wbs"], c["abs"])
    d["psmax"] = int(np.abs(cc.ps16.astype(np.float64)).max())
    _coverage(c, dd, d, oc)
    if not has_codes:
        return
    mc, mp = code.cpu().numpy(), passed.cpu().numpy()
    assert mc.shape == oc.shape
    # slice pairs whose binary_mask entry is 0 (the int8 wrap at bsa * j + bsw * k >= 8: pair (2, 2) of 6 / 6 bits in
    # 2-bit slices, pair (1, 1) of 8 / 8 in 4-bit slices) touch neither the output nor any gradient; a forward may
    # skip them and record code 0 / pass 0 (the w8a8 first conv does), or evaluate them like any other pair
    nbw, nba = c["wb"] // c["wbs"], c["ab"] // c["abs"]
    live = np.broadcast_to((co.make_binary_mask(nbw, nba, c["wbs"], c["abs"]) != 0), mc.shape)
    assert np.array_equal(mc[live], oc[live]), f"ADC codes differ at {np.argwhere((mc != oc) & live)[:5].tolist()}"
    assert np.array_equal(mp[live], op[live]), f"STE pass bits differ at {np.argwhere((mp != op) & live)[:5].tolist()}"
    skipped = not mc[~live].any() and not mp[~live].any()
    assert skipped or (np.array_equal(mc[~live], oc[~live]) and np.array_equal(mp[~live], op[~live]))


# ------------------------------------------------------------------------------------------
# the forward-only modes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", FORWARD_ONLY, ids=[case_id(MODULE_CASES[i]) for i in FORWARD_ONLY])
def test_forward_only_modes_slices(cuda_device, idx):
    """the no-grad forward equals the training forward, and forward_fused the four torch ops, bit for bit"""
    c = MODULE_CASES[idx]
    d = _module_data(c, 8600 + idx, step="quantile")
    m, = _modules(c, d, cuda_device, oracle=False)
    _assert_route(c, m, d["x"].shape)
    L = _L()
    assert route_names(L, make_desc(L, c, options=L.CIMQ_OPT_INFERENCE)) == (c["route"][0], "none", "none")
    x = torch.from_numpy(d["x"]).to(cuda_device)
    train_out = m(x.clone().requires_grad_(True)).detach()
    v = _plain(m, x)
    ho, wo = out_hw(c)
    assert tuple(v.shape) == (c["B"], c["O"], ho, wo)
    assert torch.equal(v, train_out), float((v - train_out).abs().max())
    scale, shift, res = _tables(v, 460 + idx)
    got = _fused(m, x, scale, shift, residual=res, relu=True)
    want = _ref(v, scale, shift, res, True)
    assert got.shape == v.shape and torch.equal(got, want), float((got - want).abs().max())
    assert torch.equal(_fused(m, x, scale, shift), _ref(v, scale, shift))
    frac = float((want == 0).float().mean())
    assert 0.05 < frac < 0.95, frac  # (ReLU does cut, and not everything)


# ------------------------------------------------------------------------------------------
# activation codes
# ------------------------------------------------------------------------------------------
def _layer(c, cin, cout, dev, x, seed):
    """a fresh Conv2dLSQCiM cin -> cout (3 x 3, pad 1) at the case's bit and slice widths, after its first-step
    initialisation on input x"""
    import cim_quantization_amd._modules as my_nn
    torch.manual_seed(seed)
    m = my_nn.Conv2dLSQCiM(cin, cout, 3, 1, 1, bias=False, **_kw(c["wb"], c["xbar"], c["adc"], c["ab"], c["wbs"],
                                                                 c["abs"]))
    torch.nn.init.kaiming_normal_(m.weight)
    m = m.to(dev).train()
    m(x)
    return m


@pytest.mark.parametrize("idx", CODE_CASES, ids=[case_id(MODULE_CASES[i]) for i in CODE_CASES])
def test_codes_in_and_out_slices(cuda_device, idx):
    """the codes the forward's epilogue writes for a consumer with multi-bit activation slices equal the torch
    quantiser's, and a layer fed its input as codes gives the output it gives on the fp32 tensor (the code -> word
    table of the prologue at this slice width), bit for bit"""
    c = MODULE_CASES[idx]
    d = _module_data(c, 8600 + idx, step="quantile")
    m, = _modules(c, d, cuda_device, oracle=False)
    _assert_route(c, m, d["x"].shape)
    x = torch.from_numpy(d["x"]).to(cuda_device)
    assert _ready(m, x) == codes_expected(c) == (True, True)
    v = _plain(m, x)
    scale, shift, res = _tables(v, 560 + idx)
    ep = dict(residual=res, relu=True)
    y = _fused(m, x, scale, shift, **ep)
    # output codes: the consumer's step size from a quantile of the positive outputs, Qp - 0.5 steps to their 92 %
    # point, so that a few per cent of the codes sit at Qp and the codes below occur
    qp = 2 ** c["ab"] - 1
    cons = _layer(c, c["O"], 16, cuda_device, y, 570 + idx)
    pos = y[y > 0].float().cpu()
    with torch.no_grad():
        cons.alpha_act.fill_(float(torch.quantile(pos[:1_000_000], 0.92)) / (qp - 0.5))
    assert cons.abitslice == c["abs"] and cons.nbits_a == c["ab"]
    want = _twin(cons, y)
    frac0, fracq = float((want == 0).float().mean()), float((want == qp).float().mean())
    present = set(want.view(-1).tolist())
    print(f"codes 0: {frac0:.3f}, codes Qp: {fracq:.3f}, {len(present)} of {qp + 1} codes present")
    assert present == set(range(qp + 1))
    assert 0.05 < frac0 < 0.80 and fracq >= 0.01
    yf, q = _fused(m, x, scale, shift, out_quant=cons, **ep)
    assert q.dtype == torch.uint8 and q.shape == y.shape and torch.equal(yf, y)
    assert torch.equal(q.cpu(), want)
    assert torch.equal(_fused(m, x, scale, shift, out_quant=cons, keep_float=False, **ep).cpu(), want)
    # ... and the consumer reads them: codes in equal fp32 in
    assert _ready(cons, y)[0]
    s2, t2, r2 = _tables(_plain(cons, y), 580 + idx)
    assert torch.equal(_fused(cons, q, s2, t2, residual=r2, relu=True), _fused(cons, y, s2, t2, residual=r2, relu=True))
    # input codes of the case layer itself, every code 0 .. Qp (and Qp + 1 for NaN) among them
    for nans in (False, True):
        xx = x.clone()
        if nans:
            _plant_nans(xx)
        xq = m.act_codes(xx.cpu()).to(cuda_device)
        assert set(xq.view(-1).tolist()) == set(range(qp + (2 if nans else 1)))
        for e in (dict(), ep):
            got, ref = _fused(m, xq, scale, shift, **e), _fused(m, xx, scale, shift, **e)
            assert got.dtype == torch.float32
            assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), (nans, e.keys())


def test_net_plan_two_layers_slices(cuda_device):
    """one cimq_net_forward plan of two 4 / 4-bit layers with 2-bit slices, the second reading the first's codes
    and its fp32 plane as the residual: every plane equals the loop of forward_fused calls (test_gpu_net's
    test_layer_planes)"""
    from test_gpu_net import _Plan, _bits
    c = MODULE_CASES[CODE_CASES[0]]
    assert (c["wb"], c["ab"], c["wbs"], c["abs"]) == (4, 4, 2, 2)
    d = _module_data(c, 8600 + CODE_CASES[0], step="quantile")
    m, = _modules(c, d, cuda_device, oracle=False)
    _assert_route(c, m, d["x"].shape)
    x = torch.from_numpy(d["x"]).to(cuda_device)
    s1, t1, _ = _tables(_plain(m, x), 590)
    y1 = _fused(m, x, s1, t1, relu=True)
    cons = _layer(c, c["O"], c["O"], cuda_device, y1, 591)
    with torch.no_grad():
        cons.alpha_act.fill_(float(torch.quantile(y1[y1 > 0].float().cpu(), 0.92)) / (2 ** c["ab"] - 1.5))
    s2, t2, _ = _tables(_plain(cons, y1), 592)
    L = _L()
    try:
        m.eval()
        cons.eval()
        yf, q = _fused(m, x, s1, t1, relu=True, out_quant=cons)
        assert torch.equal(yf, y1) and int(q.max()) == 2 ** c["ab"] - 1
        want2 = _fused(cons, q, s2, t2, residual=y1, relu=True)
        p = _Plan(x)
        a = p.slot(y1.shape, codes=True)
        b = p.slot(want2.shape)
        p.layer(m, x.shape, s1, t1, True, -1, a, out_mode=3, consumer=1)
        p.layer(cons, y1.shape, s2, t2, True, a, b, in_codes=1, res_slot=a)
        for it in p.items:
            assert (it["desc"].bs_w, it["desc"].bs_a) == (2, 2) and route_names(L, it["desc"])[0] == "v3"
        runs = []
        for _ in range(2):  # twice on the same buffers
            p.run()
            runs.append((p.sf[a].clone(), p.sc[a].clone(), p.sf[b].clone()))
    finally:
        m.train()
        cons.train()
    for got in runs:
        assert torch.equal(_bits(got[0]), _bits(y1))
        assert torch.equal(got[1], q)
        assert torch.equal(_bits(got[2]), _bits(want2))


# ------------------------------------------------------------------------------------------
# the shift ADC module
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,supported", SHIFT_CASES, ids=[case_id(c) for c, _ in SHIFT_CASES])
def test_shift_module_vs_oracle_slices(cuda_device, monkeypatch, c, supported):
    """Conv2dLSQCiM(adc_shift=True) with 2-bit slices, with test_gpu_shift_fullbatch's assertions (grad_beta and
    run-to-run bit identity included): on libcimq's fused shift path at xbar 128 (psmax = 128 * 4 * 4 = 2048, the
    largest the path's threshold search admits) and xbar 64, and on the general kernels one step off it (O = 24)"""
    import ctypes

    from cim_quantization_amd import functional as F
    from test_gpu_shift_fullbatch import _check
    L = _L()
    d = make_desc(L, c, variant=L.CIMQ_ADC_SHIFT_ROUND)
    assert L.load().cimq_module_shift_supported(ctypes.byref(d)) == supported
    assert route_names(L, d) == c["route"]
    assert c["wb"] == c["ab"] and c["wbs"] == c["abs"] and c["H"] == c["W"]
    m = _check(cuda_device, monkeypatch, c["C"], c["O"], c["H"], c["s"][0], c["wb"], c["B"], 9600 + c["O"] + c["xbar"],
               signed=False, xbar=c["xbar"], bs=c["wbs"])
    assert (m.wbitslice, m.abitslice) == (c["wbs"], c["abs"])
    assert bool(m._shift_fused(torch.empty(c["B"], c["C"], c["H"], c["W"], device=cuda_device))) == bool(supported)
    desc, _ = F._shift_module_descs((c["B"], c["C"], c["H"], c["W"]), m.weight, m.stride, m.padding, m.dilation,
                                    m.nbits_a, m.abitslice, m.nbits_w, m.wbitslice, m.xbar, m.nbits_alpha)
    assert (desc.bs_w, desc.bs_a) == (c["wbs"], c["abs"]) and route_names(L, desc) == c["route"]
