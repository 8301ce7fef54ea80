"""Wide module layers trained under Conv2dLSQCiM.wide_backward (CIMQ_OPT_WIDE_BWD): the state-writing wide forward,
cim_bwd_gx_wide_kernel and cim_bwd_gw_wide_kernel against the module oracle, with test_gpu_wide's data builder,
coverage assertions and bounds (1e-5 of max(|ref|, sum |terms|); 1e-5 * t_act for alpha_act)."""
import math

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import cim_oracle as co
from rect_cases import route_names
from test_gpu_fullsize import _capture_oracle_ctx, _lsq_scalar_terms, _oracle_codes
from test_gpu_rect import _module_data, _modules
from test_gpu_wide import _coverage, _two_bit_weight_step
from wide_bwd_cases import B1, CASES, LITERAL, WIDE_BWD
from wide_cases import WIDE, case_id

pytestmark = pytest.mark.gpu

_DATA = {}
PARAMS = ("weight", "alpha_act", "alpha_weight", "alpha_cim")


def _case(idx, dev):
    c = CASES[idx]
    if idx not in _DATA:
        _DATA[idx] = _module_data(c, 9900 + idx, step="quantile")
        if c["wb"] == 2:
            _DATA[idx] = _two_bit_weight_step(c, _DATA[idx], 9950 + idx)
    d = _DATA[idx]
    m, om = _modules(c, d, dev)
    return c, d, m, om


def _run(m, x, g, dev, wide):
    """forward + backward of m on fresh gradients; (out, grad_x, parameter gradients)"""
    m.wide_backward = wide
    for n in PARAMS:
        getattr(m, n).grad = None
    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    out = m(xt)
    out.backward(torch.from_numpy(g).to(dev))
    torch.cuda.synchronize()
    return out.detach(), xt.grad, [getattr(m, n).grad.clone() for n in PARAMS]


def _routes(m, x_shape):
    import cim_quantization_amd._lib as L
    from cim_quantization_amd import functional as F
    return route_names(L, F.module_descs(m, tuple(x_shape))[0])


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_backward_vs_oracle(cuda_device, monkeypatch, idx):
    c, d, m, om = _case(idx, cuda_device)
    x, w, g = d["x"], d["w"], d["g"]
    out0, _, _ = _run(m, x, g, cuda_device, False)
    assert _routes(m, x.shape) == WIDE
    out, gx, pg = _run(m, x, g, cuda_device, True)
    assert _routes(m, x.shape) == WIDE_BWD
    assert torch.equal(out, out0)  # the state instances add in the stateless instances' order

    box = _capture_oracle_ctx(monkeypatch)
    ox = torch.from_numpy(x).requires_grad_(True)
    oout = om(ox)
    cc = box["c"]
    bm = om.binary_mask.numpy()
    terms = (np.abs(cc.adc.astype(np.float64)) * np.abs(bm.astype(np.float64))).sum(axis=(1, 2, 3))
    terms = terms.transpose(0, 2, 1).reshape(oout.shape)
    assert rel_err(out.cpu().numpy(), oout.detach().numpy(), terms) < 1e-5
    dd = om.dbg
    alpha_q = co.alpha_quantize(om.alpha_cim.detach().numpy(), 8)
    oc, _ = _oracle_codes(dd["x_q"].detach().numpy(), dd["w_q"].detach().numpy(), c["s"], c["p"], c["wb"], c["xbar"],
                          alpha_q, dd["sw"].detach().numpy().reshape(1), dd["sa"].detach().numpy().reshape(1), 0.0,
                          ab=c["ab"], wbs=c["wbs"], abs_=c["abs"])
    _coverage(c, dd, d, oc)
    oout.backward(torch.from_numpy(g))
    B, O = g.shape[:2]
    g_bpo = np.ascontiguousarray(g.reshape(B, O, -1).transpose(0, 2, 1))
    ax, aw, aa = co.cim_backward(cc, g_bpo, absolute=True)
    np_ = lambda t: t.detach().cpu().numpy()  # noqa: E731
    errs = dict(grad_x=rel_err(np_(gx), np_(ox.grad), ax.reshape(x.shape)),
                grad_w=rel_err(np_(pg[0]), np_(om.weight.grad), aw.reshape(w.shape)))
    t_act = _lsq_scalar_terms(x, dd["x_q"].grad.numpy(), dd["sa"].item(), 0, d["qp_a"],
                              1.0 / math.sqrt(x.size * d["qp_a"]))
    d_act = abs(pg[1].item() - om.alpha_act.grad.item())
    # alpha_cim (test_gpu_parity's form: the entries at the quantiser's max / min carry the scale's chain) and
    # alpha_weight against its absolute-term sum
    ga, gr = np_(pg[3]), np_(om.alpha_cim.grad)
    a = om.alpha_cim.detach().numpy()
    inner = (a != a.max()) & (a != a.min())
    errs["grad_alpha_cim"] = rel_err(ga[inner], gr[inner], np.broadcast_to(aa, gr.shape)[inner])
    assert np.abs(ga - gr).max() <= 1e-5 * np.abs(gr).max(), "grad_alpha_cim (max / min entries)"
    t_w = _lsq_scalar_terms(w, dd["w_q"].grad.numpy(), dd["sw"].item(), d["qn_w"], d["qp_w"],
                            1.0 / math.sqrt(w.size * d["qp_w"]))
    assert abs(pg[2].item() - om.alpha_weight.grad.item()) <= 1e-5 * t_w
    print(f"{case_id(c)}: {errs}, alpha_act {d_act:.3e} of {t_act:.3e}")
    assert all(e < 1e-5 for e in errs.values()), errs
    assert d_act <= 1e-5 * t_act
    # a second run with the option: every bit again
    out2, gx2, pg2 = _run(m, x, g, cuda_device, True)
    assert torch.equal(out2, out) and torch.equal(gx2, gx)
    assert all(torch.equal(a, b) for a, b in zip(pg2, pg))


@pytest.mark.parametrize("idx", LITERAL, ids=[case_id(CASES[i]) for i in LITERAL])
def test_literal_flag(cuda_device, idx):
    """B6: an all-equal alpha_cim (scale 0, alpha_q NaN) sets the literal flag, so the state words come from the
    per-pair loop's ste_literal / code_literal -- at w3a3 one word, at w4a4 the word pair.  out keeps the stateless
    instance's bits; every tensor gradient read from those words has the module oracle's NaN pattern and its finite
    entries within 1e-5 of the oracle's largest (test_gpu_alpha_equal's comparison, which the v7 kernels meet on theirs)"""
    from test_gpu_alpha_equal import _same
    c, d, m, om = _case(idx, cuda_device)
    with torch.no_grad():
        m.alpha_cim.fill_(0.05)
        om.alpha_cim.fill_(0.05)
    out0, _, _ = _run(m, d["x"], d["g"], cuda_device, False)
    out, gx, pg = _run(m, d["x"], d["g"], cuda_device, True)
    assert _routes(m, d["x"].shape) == WIDE_BWD
    assert torch.isnan(out).all() and torch.equal(out.view(torch.int32), out0.view(torch.int32))
    ox = torch.from_numpy(d["x"]).requires_grad_(True)
    oout = om(ox)
    oout.backward(torch.from_numpy(d["g"]))
    _same(out, oout, "out")
    _same(gx, ox.grad, "grad_x")
    _same(pg[0], om.weight.grad, "grad_weight")
    _same(pg[3], om.alpha_cim.grad, "grad_alpha_cim")
    # the two scalars are sums with cancellation: against their absolute-term sums, as in the parity test
    dd, x, w = om.dbg, d["x"], d["w"]
    t_act = _lsq_scalar_terms(x, dd["x_q"].grad.numpy(), dd["sa"].item(), 0, d["qp_a"],
                              1.0 / math.sqrt(x.size * d["qp_a"]))
    t_w = _lsq_scalar_terms(w, dd["w_q"].grad.numpy(), dd["sw"].item(), d["qn_w"], d["qp_w"],
                            1.0 / math.sqrt(w.size * d["qp_w"]))
    for i, n, t in ((1, "alpha_act", t_act), (2, "alpha_weight", t_w)):
        mine, ref = pg[i].item(), getattr(om, n).grad.item()
        assert (math.isnan(mine) and math.isnan(ref)) or abs(mine - ref) <= 1e-5 * t, (n, mine, ref, t)


@pytest.mark.parametrize("defer", [False, True], ids=["accumulate", "defer_gw"])
def test_accumulate_and_deferred_grad_w(cuda_device, defer):
    """CIMQ_LSQ_ACCUMULATE_GRADS into zeroed .grad buffers, alone and with grad_w deferred to a second stream
    (CIMQ_LSQ_DEFER_GW, Route::gw_own): the plain call's gradients bit for bit.  Unchained, as test_gpu_w4a4 compares
    them: the chained epilogue packs its scalar sums in another order."""
    import cim_quantization_amd.functional as F
    c, d, m, _ = _case(B1, cuda_device)
    _, gx, pg = _run(m, d["x"], d["g"], cuda_device, True)
    assert _routes(m, d["x"].shape) == WIDE_BWD
    m.accumulate_grads_in_place = True
    m.tail_stream = torch.cuda.Stream() if defer else None
    F.CHAIN_EPILOGUES = False
    try:
        for n in PARAMS:
            getattr(m, n).grad = torch.zeros_like(getattr(m, n))
        xt = torch.from_numpy(d["x"]).to(cuda_device).requires_grad_(True)
        m(xt).backward(torch.from_numpy(d["g"]).to(cuda_device))
        torch.cuda.synchronize()
    finally:
        F.CHAIN_EPILOGUES = True
        m.accumulate_grads_in_place = False
        m.tail_stream = None
    assert torch.equal(xt.grad, gx)
    for n, ref in zip(PARAMS, pg):
        assert torch.equal(getattr(m, n).grad, ref), n


def test_harness_step_with_wide_backward(cuda_device, tmp_path, capsys, monkeypatch):
    """VGG-small at B = 2 through harness.train, three steps with and without --wide-backward, at lr 1e-4.  The first
    step initialises on the torch path and the second is the first library backward, so the third loss is the first
    behind the new gradients.  Both backwards sit within 1e-5 of their term sums of one oracle (above, and
    test_gpu_wide), so one update at lr 1e-4 leaves the two runs' weights at most ~1e-9 of a quantiser step apart: among
    4.6 M weights no code is expected to flip, and the losses differ by fp32 rounding of one forward -- bound 1e-4 of
    the loss.  (At the prototxt's lr 0.01 this B = 2 run has diverged to a loss near 80 by step three and is no
    yardstick.)  On the model that trained: the five wide layers' routes, the first conv's (general without the flag,
    c1w with it) and every parameter's gradient."""
    import cim_quantization_amd._lib as L
    from cim_quantization_amd import functional as F
    from cim_quantization_amd._modules.lsq import Conv2dLSQCiM
    from cim_quantization_amd.harness import train
    from test_gpu_harness import _data
    from test_gpu_wide import VGG_PROTO
    _data(str(tmp_path))
    built = []
    real = train.build_model
    monkeypatch.setattr(train, "build_model", lambda *a, **k: built.append(real(*a, **k)) or built[-1])
    losses = []
    for tag, flags in (("off", []), ("on", ["--wide-backward"])):
        hp = tmp_path / (tag + ".prototxt")
        proto = VGG_PROTO.format(log=str(tmp_path / tag), data=str(tmp_path), extra="")
        hp.write_text(proto.replace("batch_size: 8", "batch_size: 2").replace("lr: 0.01", "lr: 0.0001"))
        train.main(["--hp", str(hp), "--max-steps", "3", "--max-val-steps", "1"] + flags)
        out = capsys.readouterr().out
        losses.append([float(ln.split("loss ")[1].split()[0]) for ln in out.splitlines() if ln.startswith("Epoch [")])
    # (the w8a8 first conv, 3 -> 128 on 32 x 32, trains on cim_bwd_c1w_kernel with the flag: test_gpu_c1w)
    for (model, _), want, want1 in zip(built, (WIDE, WIDE_BWD), (("v3", "general", "general"), ("v3", "c1w", "c1w"))):
        wide = [m for m in model.modules() if isinstance(m, Conv2dLSQCiM) and m.in_channels >= 128]
        assert len(wide) == 5
        for m in wide:
            assert route_names(L, F.module_descs(m, m._last_x_shape)[0]) == want
        first = [m for m in model.modules() if isinstance(m, Conv2dLSQCiM) and m.in_channels == 3]
        assert len(first) == 1 and (first[0].out_channels, first[0].nbits_w, first[0].nbits_a) == (128, 8, 8)
        assert first[0]._last_x_shape == (2, 3, 32, 32)
        assert route_names(L, F.module_descs(first[0], first[0]._last_x_shape)[0]) == want1
        for n, p in model.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
    off, on = losses
    print("losses without / with the option:", off, on)
    assert len(off) == len(on) == 3 and all(np.isfinite(off + on))
    assert off[:2] == on[:2]
    assert abs(on[2] - off[2]) <= 1e-4 * abs(off[2])
