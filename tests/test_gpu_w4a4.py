"""GPU: w4a4 layers in 1-bit slices -- four slices a side, 16 slice pairs -- on the compact-state backward.

The training forward (cim_fwd_v3_kernel, CST 4) writes one 8-byte state word per (tile, pixel, channel): two of the
v7 words, the pairs of weight slices 0-1 and 2-3.  cim_bwd_gx_v8_kernel<4, 4, ..> and cim_bwd_gw_v7_kernel<4, 4, ..>
read them.  The cases and the route each must take are w4a4_cases.py's (test_w4a4_routes_host.py asserts the routes on
the CPU too), and every case asserts its route before it launches: on a library without the format the module and
Function cases stop there (it answers the general backward), and debug_state_codes refuses the layer.

Bars, the suite's own: integer partial sums and ADC outputs bit-exact; out within 1e-6 and the gradients within 1e-5 of
max(|ref|, sum of |terms|) element by element; step-size gradients within 1e-5 of the sum of |terms|; ADC codes and
STE-pass bits of the state words equal to the oracle's; the forward-only modes torch.equal.
"""
import math

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import cim_oracle as co
from rect_cases import make_desc, out_hw, route_names
from test_gpu_codes import _plant_nans, _ready, _twin
from test_gpu_epilogue import _fused, _plain, _ref, _tables
from test_gpu_fullsize import _capture_oracle_ctx, _check_elementwise, _lsq_scalar_terms, _oracle_codes
from test_gpu_parity import _check_integer_steps, _random_inputs, _sampled_images_and_properties, run_hip_function
from test_gpu_rect import _assert_route, _module_data, _modules
from test_gpu_slices import _layer
from w4a4_cases import (ADC_CASES, BAND_CASE, FORWARD_ONLY, FUNCTION_CASES, LITERAL_CASE, MODULE_CASES, V7, case_id)

pytestmark = pytest.mark.gpu


def _L():
    import cim_quantization_amd._lib as L
    return L


def _assert_desc_route(c):
    L = _L()
    assert c["route"] == V7 and route_names(L, make_desc(L, c)) == V7


# ------------------------------------------------------------------------------------------
# the module path, steady state
# ------------------------------------------------------------------------------------------
def _coverage(c, dd, d, oc, op):
    """conditions on the oracle's values, so that a dead top slice cannot hide a fault: every slice pair's ADC codes
    vary and its STE mask cuts, activations reach Qp and the weights both clamp ends"""
    nz = (oc != 0).mean(axis=(0, 1, 4, 5))  # per (k, j)
    cl = (op == 0).mean(axis=(0, 1, 4, 5))
    xr = np.rint(dd["x_q"].detach().numpy() / dd["sa"].item())
    wr = np.rint(dd["w_q"].detach().numpy() / dd["sw"].item())
    at_qp = (np.abs(xr) == d["qp_a"]).mean()
    print(f"{case_id(c)}: nonzero codes per slice pair {nz.min():.3f} .. {nz.max():.3f}, clamped partial sums "
          f"{cl.min():.3f} .. {cl.max():.3f}, activations at Qp {at_qp:.4f}, weights at Qn "
          f"{(wr == d['qn_w']).mean():.4f}, at Qp {(wr == d['qp_w']).mean():.4f}")
    assert nz.shape == (4, 4) and nz.min() >= 0.05 and nz.max() <= 0.95, nz
    assert cl.min() >= 0.02, cl
    assert at_qp >= 0.01
    assert (wr == d["qn_w"]).any() and (wr == d["qp_w"]).any()


def _run_module(m, x, g, dev):
    from cim_quantization_amd import functional as F
    for p in m.parameters():
        p.grad = None
    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    out = m(xt)
    code, passed = F.debug_state_codes(out)
    out.backward(torch.from_numpy(g).to(dev))
    torch.cuda.synchronize()
    grads = [xt.grad.clone()] + [p.grad.clone() for p in m.parameters() if p.grad is not None]
    return xt, out, code.clone(), passed.clone(), grads


@pytest.mark.parametrize("idx", range(len(MODULE_CASES)), ids=[case_id(c) for c in MODULE_CASES])
def test_module_vs_oracle_w4a4(cuda_device, monkeypatch, idx):
    """Conv2dLSQCiM in steady state against the module oracle on the whole batch, asserted as
    test_gpu_slices.test_module_vs_oracle_slices does; the state words' codes and pass bits element by element; and
    a second run of the same step, bit for bit"""
    c = MODULE_CASES[idx]
    d = _module_data(c, 9400 + idx, step="quantile")
    m, om = _modules(c, d, cuda_device)
    assert (m.nbits_w, m.nbits_a, m.wbitslice, m.abitslice) == (4, 4, 1, 1)
    x, w, g = d["x"], d["w"], d["g"]
    _assert_route(c, m, x.shape)
    ho, wo = out_hw(c)

    xt, out, code, passed, grads = _run_module(m, x, g, cuda_device)
    assert tuple(out.shape) == (c["B"], c["O"], ho, wo) and out.is_contiguous()

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
    oc, op = _oracle_codes(dd["x_q"].detach().numpy(), dd["w_q"].detach().numpy(), c["s"], c["p"], 4, c["xbar"],
                           alpha_q, sw_np, sa_np, float(c["signed"]))
    _coverage(c, dd, d, oc, op)
    mc, mp = code.cpu().numpy(), passed.cpu().numpy()
    assert mc.shape == oc.shape
    assert np.array_equal(mc, oc), f"ADC codes differ at {np.argwhere(mc != oc)[:5].tolist()}"
    assert np.array_equal(mp, op), f"STE pass bits differ at {np.argwhere(mp != op)[:5].tolist()}"

    _, out2, code2, passed2, grads2 = _run_module(m, x, g, cuda_device)
    assert torch.equal(out2, out) and torch.equal(code2, code) and torch.equal(passed2, passed)
    assert len(grads) == len(grads2) >= 5  # grad_x, weight, alpha_act, alpha_weight, alpha_cim
    for a, b in zip(grads, grads2):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------
# the Function path ([B, P, O]); the other ADC modes; another binary_mask
# ------------------------------------------------------------------------------------------
def _function_case(dev, cfg, seed, alter_mask=False):
    inp = _random_inputs(cfg, seed)
    assert inp["binary_mask"].shape[2:4] == (4, 4)
    if alter_mask:
        # pair (k, j) = (1, 2): 2^(k + j) = 8 becomes 3, so neither E_k nor D_j is a popcount times a power of two
        bm = inp["binary_mask"].copy()
        assert bm[0, 0, 1, 2, 0, 0] == 8
        bm[0, 0, 1, 2, 0, 0] = 3
        inp["binary_mask"] = bm
    out, c = co.cim_forward(inp["x_q"], inp["w_q"], cfg["s"], cfg["p"], (1, 1), 4, 1, 4, 1, cfg["adc"], cfg["xbar"],
                            inp["binary_mask"], inp["alpha_q"], inp["sw"], inp["sa"], False, inp["signed_act"],
                            return_debug=True)
    gx, gw, ga = co.cim_backward(c, inp["grad"])
    ax, aw, aa = co.cim_backward(c, inp["grad"], absolute=True)
    res = run_hip_function(dev, cfg, inp)
    _check_integer_steps(cfg, inp, res, c.ps16)
    out_terms = np.sum(np.abs(c.adc.astype(np.float64) * inp["binary_mask"]), axis=(1, 2, 3))
    assert res["out"].shape == out.shape and res["grad_x"].shape == gx.shape and res["grad_w"].shape == gw.shape
    assert rel_err(res["out"], out, out_terms) < 1e-6
    assert rel_err(res["grad_x"], gx, ax) < 1e-5
    assert rel_err(res["grad_w"], gw, aw) < 1e-5
    assert (ga is not None) == (cfg["adc"] in (1, 1.5))
    if ga is not None:
        assert rel_err(res["grad_alpha"], ga, aa) < 1e-5


@pytest.mark.parametrize("idx", range(len(FUNCTION_CASES)), ids=[case_id(c) for c in FUNCTION_CASES])
def test_function_vs_oracle_w4a4(cuda_device, idx):
    """get_cim_output_signed on [B, P, O] against cim_forward / cim_backward (the Function form of the descriptor:
    grad_out in [B, P, O])"""
    cfg = FUNCTION_CASES[idx]
    _assert_desc_route(cfg)
    _function_case(cuda_device, cfg, 9420 + idx)


def test_function_other_binary_mask_w4a4(cuda_device):
    """one binary_mask entry altered: the backward takes the per-pair coefficient sums for E_k and D_j"""
    cfg = FUNCTION_CASES[0]
    _assert_desc_route(cfg)
    _function_case(cuda_device, cfg, 9430, alter_mask=True)


@pytest.mark.parametrize("idx", range(len(ADC_CASES)), ids=[case_id(c) for c in ADC_CASES])
def test_function_other_adc_modes_w4a4(cuda_device, idx):
    """a multi-bit ADC (no alpha_cim: pass bits only) and the sign ADC: the forward's per-pair write path"""
    cfg = ADC_CASES[idx]
    _assert_desc_route(cfg)
    _function_case(cuda_device, cfg, 9440 + idx)


def test_literal_flag_w4a4(cuda_device):
    """test_gpu_alpha_equal's all-equal alpha_cim at 4 bits: the literal ADC through the CST 4 forward's per-pair
    path, the oracle's NaN pattern and its finite entries at that test's bar"""
    from test_gpu_alpha_equal import test_module_all_equal_alpha
    c = LITERAL_CASE
    _assert_desc_route(c)
    assert (c["B"], c["C"], c["O"], c["H"], c["W"], c["kh"], c["wb"], c["xbar"]) == (2, 16, 16, 16, 16, 3, 4, 64)
    test_module_all_equal_alpha(cuda_device, 2, 16, 16, 16, 3, 4, 64)


def test_partial_grad_x_band_w4a4(cuda_device):
    """test_gpu_rect.test_partial_grad_x_band's layer at 4 bits: an 8-row and a partial 4-row grad_x band, on
    sampled images"""
    c = BAND_CASE
    _assert_desc_route(c)
    assert c["B"] * math.ceil(c["H"] / 8) >= 256 and c["H"] % 8 == 4
    _sampled_images_and_properties(cuda_device, c, 9450)


# ------------------------------------------------------------------------------------------
# the forward-only contract
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", FORWARD_ONLY, ids=[case_id(MODULE_CASES[i]) for i in FORWARD_ONLY])
def test_forward_only_modes_w4a4(cuda_device, idx):
    """the no-grad forward (the per-k family, as before) equals the training forward (CST 4), and forward_fused the
    four torch ops, bit for bit"""
    c = MODULE_CASES[idx]
    d = _module_data(c, 9400 + idx, step="quantile")
    m, = _modules(c, d, cuda_device, oracle=False)
    _assert_route(c, m, d["x"].shape)
    L = _L()
    assert route_names(L, make_desc(L, c, options=L.CIMQ_OPT_INFERENCE)) == ("v3", "none", "none")
    x = torch.from_numpy(d["x"]).to(cuda_device)
    train_out = m(x.clone().requires_grad_(True)).detach()
    v = _plain(m, x)
    ho, wo = out_hw(c)
    assert tuple(v.shape) == (c["B"], c["O"], ho, wo)
    assert torch.equal(v, train_out), float((v - train_out).abs().max())
    scale, shift, res = _tables(v, 470 + idx)
    got = _fused(m, x, scale, shift, residual=res, relu=True)
    want = _ref(v, scale, shift, res, True)
    assert got.shape == v.shape and torch.equal(got, want), float((got - want).abs().max())
    assert torch.equal(_fused(m, x, scale, shift), _ref(v, scale, shift))
    frac = float((want == 0).float().mean())
    assert 0.05 < frac < 0.95, frac  # (ReLU does cut, and not everything)


def test_codes_in_and_out_w4a4(cuda_device):
    """shape 0: the codes the epilogue writes for a 4-bit consumer equal the torch quantiser's, and the layer fed
    its input as codes gives the output it gives on the fp32 tensor, bit for bit"""
    c = MODULE_CASES[0]
    d = _module_data(c, 9400, step="quantile")
    m, = _modules(c, d, cuda_device, oracle=False)
    _assert_route(c, m, d["x"].shape)
    x = torch.from_numpy(d["x"]).to(cuda_device)
    assert _ready(m, x) == (True, True)
    v = _plain(m, x)
    scale, shift, res = _tables(v, 480)
    ep = dict(residual=res, relu=True)
    y = _fused(m, x, scale, shift, **ep)
    qp = 15
    cons = _layer(c, c["O"], 16, cuda_device, y, 481)
    pos = y[y > 0].float().cpu()
    with torch.no_grad():
        cons.alpha_act.fill_(float(torch.quantile(pos[:1_000_000], 0.92)) / (qp - 0.5))
    want = _twin(cons, y)
    assert set(want.view(-1).tolist()) == set(range(qp + 1)) and float((want == qp).float().mean()) >= 0.01
    yf, q = _fused(m, x, scale, shift, out_quant=cons, **ep)
    assert q.dtype == torch.uint8 and q.shape == y.shape and torch.equal(yf, y)
    assert torch.equal(q.cpu(), want)
    assert _ready(cons, y)[0]
    s2, t2, r2 = _tables(_plain(cons, y), 482)
    assert torch.equal(_fused(cons, q, s2, t2, residual=r2, relu=True), _fused(cons, y, s2, t2, residual=r2, relu=True))
    for nans in (False, True):
        xx = x.clone()
        if nans:
            _plant_nans(xx)
        xq = m.act_codes(xx.cpu()).to(cuda_device)
        assert set(xq.view(-1).tolist()) == set(range(qp + (2 if nans else 1)))
        for e in (dict(), ep):
            got, ref = _fused(m, xq, scale, shift, **e), _fused(m, xx, scale, shift, **e)
            assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), (nans, e.keys())


def test_net_plan_two_layers_w4a4(cuda_device):
    """one cimq_net_forward plan of two w4a4 layers, the second reading the first's codes and its fp32 plane as the
    residual: every plane equals the loop of forward_fused calls"""
    from test_gpu_net import _Plan, _bits
    c = MODULE_CASES[0]
    d = _module_data(c, 9400, step="quantile")
    m, = _modules(c, d, cuda_device, oracle=False)
    _assert_route(c, m, d["x"].shape)
    x = torch.from_numpy(d["x"]).to(cuda_device)
    s1, t1, _ = _tables(_plain(m, x), 490)
    y1 = _fused(m, x, s1, t1, relu=True)
    cons = _layer(c, c["O"], c["O"], cuda_device, y1, 491)
    with torch.no_grad():
        cons.alpha_act.fill_(float(torch.quantile(y1[y1 > 0].float().cpu(), 0.92)) / (2 ** 4 - 1.5))
    s2, t2, _ = _tables(_plain(cons, y1), 492)
    L = _L()
    try:
        m.eval()
        cons.eval()
        yf, q = _fused(m, x, s1, t1, relu=True, out_quant=cons)
        assert torch.equal(yf, y1) and int(q.max()) == 15
        want2 = _fused(cons, q, s2, t2, residual=y1, relu=True)
        p = _Plan(x)
        a = p.slot(y1.shape, codes=True)
        b = p.slot(want2.shape)
        p.layer(m, x.shape, s1, t1, True, -1, a, out_mode=3, consumer=1)
        p.layer(cons, y1.shape, s2, t2, True, a, b, in_codes=1, res_slot=a)
        for it in p.items:
            assert (it["desc"].bits_w, it["desc"].bs_w) == (4, 1) and route_names(L, it["desc"]) == ("v3", "none", "none")
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
# training plumbing: prepared weights, chained epilogues, the deferred grad_w
# ------------------------------------------------------------------------------------------
SPECS = [(16, 16, 16, 1), (16, 32, 16, 2)]  # (C, O, H, stride): shapes 0 and 2


def _stack(dev, overlap=False):
    import cim_quantization_amd._modules as my_nn
    from cim_quantization_amd.dist import GradBucket
    torch.manual_seed(5)
    layers = []
    for c, o, h, s in SPECS:
        m = my_nn.Conv2dLSQCiM(c, o, 3, s, 1, bias=False, nbits_w=4, nbits_a=4, nbits_alpha=8, xbar=128, adcbits=1.5)
        torch.nn.init.kaiming_normal_(m.weight)
        layers.append(m.to(dev).train())
    bucket = GradBucket([p for m in layers for p in m.parameters()])
    bucket.own(layers, overlap=overlap)
    return layers, bucket


def _data(dev, seed, B=2):
    g = torch.Generator().manual_seed(seed)
    xs, gs = [], []
    for c, o, h, s in SPECS:
        xs.append(torch.randn(B, c, h, h, generator=g).relu().to(dev))
        ho = (h + 2 - 3) // s + 1
        gs.append((torch.randn(B, o, ho, ho, generator=g) / (B * o * ho * ho) ** 0.5).to(dev))
    return xs, gs


def _step(layers, bucket, xs, gs, chained, prepare=False):
    from cim_quantization_amd import functional as F
    if prepare:
        assert F.prepare_weights(layers) == len(layers)
    gxs = []
    bucket.zero()
    with (F.chained_epilogues() if chained else torch.enable_grad()):
        for m, x, g in zip(layers, xs, gs):
            xr = x.detach().requires_grad_(True)
            m(xr).backward(g)
            gxs.append(xr.grad)
    bucket.join()
    torch.cuda.synchronize()
    return gxs, bucket.flat.detach().clone()


def _two_stacks(dev, overlap):
    from cim_quantization_amd import functional as F
    la, ba = _stack(dev, overlap=overlap)
    lb, bb = _stack(dev)
    xs, gs = _data(dev, 9)
    for layers, bucket in ((la, ba), (lb, bb)):
        _step(layers, bucket, xs, gs, False)  # the initialising step (torch path)
        _step(layers, bucket, xs, gs, False)  # the first library step records the input shapes
    for m, x in zip(la, xs):
        assert route_names(_L(), F.module_descs(m, tuple(x.shape))[0]) == V7
    return la, ba, lb, bb


def test_prepared_chained_equals_unchained_w4a4(cuda_device):
    """two w4a4 layers under prepare_weights + chained_epilogues against the unchained, unprepared calls: grad_x bit
    for bit (same kernels, fixed-order sums), the parameter gradients to fp32 summation order (test_gpu_chain)"""
    import cim_quantization_amd.functional as F
    from test_gpu_chain import _close
    la, ba, lb, bb = _two_stacks(cuda_device, False)
    xs2, gs2 = _data(cuda_device, 10)
    F.CHAIN_EPILOGUES = False
    try:
        gx_ref, flat_ref = _step(lb, bb, xs2, gs2, False)
    finally:
        F.CHAIN_EPILOGUES = True
    gx_ch, flat_ch = _step(la, ba, xs2, gs2, True, prepare=True)
    for i, (a, b) in enumerate(zip(gx_ch, gx_ref)):
        assert torch.equal(a, b), i
    _close(flat_ch, flat_ref)
    assert torch.isfinite(flat_ch).all() and float(flat_ch.abs().max()) > 0


def test_deferred_grad_w_equals_single_stream_w4a4(cuda_device):
    """GradBucket.own(overlap=True): grad_w of the v7 layers (CIMQ_LSQ_DEFER_GW) and the epilogues on the bucket's
    second stream; same kernels, same inputs as the unchained single-stream backward: every gradient bit for bit"""
    import cim_quantization_amd.functional as F
    la, ba, lb, bb = _two_stacks(cuda_device, True)
    xs2, gs2 = _data(cuda_device, 10)
    F.CHAIN_EPILOGUES = False
    try:
        gx_ref, flat_ref = _step(lb, bb, xs2, gs2, False)
    finally:
        F.CHAIN_EPILOGUES = True
    gx_ov, flat_ov = _step(la, ba, xs2, gs2, True)
    for i, (a, b) in enumerate(zip(gx_ov, gx_ref)):
        assert torch.equal(a, b), i
    assert torch.equal(flat_ov, flat_ref)
    assert torch.isfinite(flat_ov).all()


def test_harness_trains_a_4bit_prototxt(cuda_device, tmp_path, capsys):
    """harness.train on test_gpu_harness's ResNet-20 with a prototxt that asks for 4 bits: one epoch of two steps
    with finite losses, and the 3 x 3 layers it built route to (v3, v7, v7) at its batch size"""
    import cim_quantization_amd.functional as F
    from cim_quantization_amd._modules.lsq import Conv2dLSQCiM
    from cim_quantization_amd.harness import train
    from test_gpu_harness import PROTO, _data as cifar_data
    cifar_data(str(tmp_path))
    proto = PROTO.replace("nbits_w: 3", "nbits_w: 4").replace("nbits_a: 3", "nbits_a: 4").replace("epochs: 2",
                                                                                                 "epochs: 1")
    assert "nbits_w: 4" in proto and "nbits_a: 4" in proto and "epochs: 1" in proto
    hp = tmp_path / "train4.prototxt"
    hp.write_text(proto.format(log=str(tmp_path / "run4"), data=str(tmp_path), extra=""))
    model, _ = train.build_model(train.load_hyperparam(str(hp)), cuda_device)
    convs = [(n, m) for n, m in model.named_modules() if isinstance(m, Conv2dLSQCiM) and m.nbits_w == 4]
    assert len(convs) >= 18
    sizes = {16: 32, 32: 16, 64: 8}
    for n, m in convs:
        if m.kernel_size == (3, 3) and m.stride == (1, 1):
            h = sizes[m.in_channels]
            assert route_names(_L(), F.module_descs(m, (64, m.in_channels, h, h))[0]) == V7, n
    best = train.main(["--hp", str(hp), "--max-steps", "2", "--max-val-steps", "1"])
    out = capsys.readouterr().out
    losses = [float(l.split("loss ")[1].split()[0]) for l in out.splitlines() if l.startswith("Epoch [")]
    assert len(losses) == 2 and all(np.isfinite(losses)) and np.isfinite(best)
