"""The w8a8 first conv beyond 16 output channels trained under Conv2dLSQCiM.wide_backward (CIMQ_OPT_WIDE_BWD):
cim_bwd_c1w_kernel (+ c1w_fold_kernel) against the module oracle in float64 on the same inputs, with DESIGN section 2's
bound: 1e-5 of max(|ref|, sum |terms|); 1e-5 of the term sum for the two LSQ scalars."""
import math

import numpy as np
import pytest
import torch

from c1w_cases import CASES, LITERAL, routes
from conftest import rel_err
from oracle import cim_oracle as co
from rect_cases import case_id, route_names
from test_gpu_fullsize import _capture_oracle_ctx, _lsq_scalar_terms, _oracle_codes
from test_gpu_rect import _module_data, _modules

pytestmark = pytest.mark.gpu

_DATA = {}


def _case(idx, dev):
    c = CASES[idx]
    if idx not in _DATA:
        _DATA[idx] = _module_data(c, 9700 + idx, step="quantile")
    m, om = _modules(c, _DATA[idx], dev)
    return c, _DATA[idx], m, om


def _params(m):
    return [n for n in ("weight", "alpha_act", "alpha_weight", "alpha_cim") if getattr(m, n) is not None]


def _run(m, x, g, dev, wide):
    """forward + backward of m on fresh gradients; (out, grad_x, parameter gradients by name)"""
    m.wide_backward = wide
    for n in _params(m):
        getattr(m, n).grad = None
    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    out = m(xt)
    out.backward(torch.from_numpy(g).to(dev))
    torch.cuda.synchronize()
    return out.detach(), xt.grad, {n: getattr(m, n).grad.clone() for n in _params(m)}


def _routes(m, x_shape):
    import cim_quantization_amd._lib as L
    from cim_quantization_amd import functional as F
    return route_names(L, F.module_descs(m, tuple(x_shape))[0])


def _scalar_terms(d, dd):
    x, w = d["x"], d["w"]
    t_act = _lsq_scalar_terms(x, dd["x_q"].grad.numpy(), dd["sa"].item(), 0, d["qp_a"],
                              1.0 / math.sqrt(x.size * d["qp_a"]))
    t_w = _lsq_scalar_terms(w, dd["w_q"].grad.numpy(), dd["sw"].item(), d["qn_w"], d["qp_w"],
                            1.0 / math.sqrt(w.size * d["qp_w"]))
    return t_act, t_w


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_backward_vs_oracle(cuda_device, monkeypatch, idx):
    c, d, m, om = _case(idx, cuda_device)
    x, w, g = d["x"], d["w"], d["g"]
    out0, _, _ = _run(m, x, g, cuda_device, False)
    assert _routes(m, x.shape)[1:] == ("general", "general")
    out, gx, pg = _run(m, x, g, cuda_device, True)
    assert _routes(m, x.shape) == routes(c)  # (fails on a library without the route: general != c1w)
    assert torch.equal(out, out0)

    box = _capture_oracle_ctx(monkeypatch)
    ox = torch.from_numpy(x).requires_grad_(True)
    oout = om(ox)
    cc, dd = box["c"], om.dbg
    if c["adc"] == 1.5:
        # on the oracle's values: the codes of the live slice pairs are mixed
        alpha_q = co.alpha_quantize(om.alpha_cim.detach().numpy(), 8)
        oc, _ = _oracle_codes(dd["x_q"].detach().numpy(), dd["w_q"].detach().numpy(), c["s"], c["p"], 8, c["xbar"],
                              alpha_q, dd["sw"].detach().numpy().reshape(1), dd["sa"].detach().numpy().reshape(1),
                              float(c["signed"]))
        nz = (oc != 0)[:, :, om.binary_mask.numpy().reshape(8, 8) != 0].mean()
        print(f"{case_id(c)}: nonzero codes of the live pairs {nz:.3f}")
        assert 0.05 <= nz <= 0.95
    oout.backward(torch.from_numpy(g))
    B, O = g.shape[:2]
    ax, aw, aa = co.cim_backward(cc, np.ascontiguousarray(g.reshape(B, O, -1).transpose(0, 2, 1)), absolute=True)
    np_ = lambda t: t.detach().cpu().numpy()  # noqa: E731
    errs = dict(grad_x=rel_err(np_(gx), np_(ox.grad), ax.reshape(x.shape)),
                grad_w=rel_err(np_(pg["weight"]), np_(om.weight.grad), aw.reshape(w.shape)))
    if "alpha_cim" in pg:
        # (test_gpu_parity's form: the entries at the quantiser's max / min carry the scale's chain)
        ga, gr, a = np_(pg["alpha_cim"]), np_(om.alpha_cim.grad), np_(om.alpha_cim)
        inner = (a != a.max()) & (a != a.min())
        errs["grad_alpha_cim"] = rel_err(ga[inner], gr[inner], np.broadcast_to(aa, gr.shape)[inner])
        assert np.abs(ga - gr).max() <= 1e-5 * np.abs(gr).max(), "grad_alpha_cim (max / min entries)"
    t_act, t_w = _scalar_terms(d, dd)
    d_act = abs(pg["alpha_act"].item() - om.alpha_act.grad.item())
    d_w = abs(pg["alpha_weight"].item() - om.alpha_weight.grad.item())
    print(f"{case_id(c)}: {errs}, alpha_act {d_act:.3e} of {t_act:.3e}, alpha_weight {d_w:.3e} of {t_w:.3e}")
    assert all(e < 1e-5 for e in errs.values()), errs
    assert d_act <= 1e-5 * t_act and d_w <= 1e-5 * t_w
    # a second run with the option: every bit again
    out2, gx2, pg2 = _run(m, x, g, cuda_device, True)
    assert torch.equal(out2, out) and torch.equal(gx2, gx)
    assert all(torch.equal(pg2[n], pg[n]) for n in pg)


def test_literal_flag(cuda_device):
    """an all-equal alpha_cim (scale 0, alpha_q NaN) sets the literal flag: the per-pair ste_literal / code_literal
    loop.  out keeps its bits; the tensor gradients have the oracle's NaN pattern and their finite entries within 1e-5
    of the oracle's largest (test_gpu_alpha_equal's comparison), the two scalars within 1e-5 of their term sums"""
    from test_gpu_alpha_equal import _same
    c, d, m, om = _case(LITERAL, cuda_device)
    with torch.no_grad():
        m.alpha_cim.fill_(0.05)
        om.alpha_cim.fill_(0.05)
    out0, _, _ = _run(m, d["x"], d["g"], cuda_device, False)
    out, gx, pg = _run(m, d["x"], d["g"], cuda_device, True)
    assert _routes(m, d["x"].shape) == routes(c)
    assert torch.equal(out.view(torch.int32), out0.view(torch.int32))
    ox = torch.from_numpy(d["x"]).requires_grad_(True)
    oout = om(ox)
    oout.backward(torch.from_numpy(d["g"]))
    _same(out, oout, "out")
    _same(gx, ox.grad, "grad_x")
    _same(pg["weight"], om.weight.grad, "grad_weight")
    _same(pg["alpha_cim"], om.alpha_cim.grad, "grad_alpha_cim")
    for n, t in zip(("alpha_act", "alpha_weight"), _scalar_terms(d, om.dbg)):
        mine, ref = pg[n].item(), getattr(om, n).grad.item()
        assert (math.isnan(mine) and math.isnan(ref)) or abs(mine - ref) <= 1e-5 * t, (n, mine, ref, t)
