"""The wide backward (CIMQ_OPT_WIDE_BWD) at batches whose launch plan is not the trivial one:
wide_bwd_cases.BATCH_CASES, N1 .. N4, where cim_bwd_gx_wide_kernel walks several ring steps over a band of RB = 4 or 8 input rows (a partial last
band in N3) and cim_bwd_gw_wide_kernel accumulates nstage = 2 .. 6 stages per workgroup (chunks that start mid-image
and a short last chunk in N2).  test_wide_bwd_host.py pins the plan's answers; here the gradients.

A float64 oracle of the whole batch would hold 40-85 M partial sums in several copies, so it runs on subsets.  The
backward is linear in grad_out and every parameter gradient is a sum over images: with g zero outside a set S of
images, the module oracle on x[S], g[S] -- with the factors that count the batch taken from the whole batch:
grad_scale's 1 / sqrt(x.numel() * Qp), which sets sa's fp32 value and scales grad_alpha_act
(OracleConv2dLSQCiM.act_numel), and grad_alpha_cim's 1 / sqrt(ps.numel() * Qp_adc) (the ctx's meta["ps_numel"]) --
gives the whole batch's grad_w, grad_alpha_cim, grad_alpha_weight, grad_alpha_act and grad_x[S] exactly, and grad_x is
zero elsewhere.  The step sizes the oracle used are asserted equal to the module's bit for bit.  S1 is chosen
by rule from the plan (the images of every stage position of the first, a middle, the last full and the short last
chunk, and images 0 and B - 1), S2 is 12 seeded random images off S1.  A dropped, doubled or misplaced stage of a chunk
in S1, or a wrong ring step of a band, shows against the oracle; the dense run adds bit-equality of out with the
stateless forward, run-to-run bit identity, grad_x of S1 and S2 against the oracle, and additivity over the split
S1 / complement, which catches an accumulator that depends on anything but its own terms.

Bounds: test_gpu_wide_bwd.test_backward_vs_oracle's (1e-5 of max(|ref|, sum |terms|); 1e-5 of the term sum for the
two LSQ scalars; grad_alpha_cim's max / min entries within 1e-5 of the oracle's largest entry) and, for additivity,
test_gpu_parity._sampled_images_and_properties' (1e-5 of the dense result's largest entry).
"""
import math

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import cim_oracle as co
from test_gpu_fullsize import _capture_oracle_ctx, _lsq_scalar_terms, _oracle_codes
from test_gpu_rect import _module_data, _modules
from test_gpu_wide import _coverage
from test_gpu_wide_bwd import PARAMS, _routes, _run
from wide_bwd_cases import BATCH_CASES, WIDE_BWD, batch_plan, stage_images
from wide_cases import WIDE, case_id

pytestmark = pytest.mark.gpu

_DATA = {}
N_RANDOM = 12


def _case(idx, dev):
    c = BATCH_CASES[idx]
    if idx not in _DATA:
        _DATA[idx] = _module_data(c, 9960 + idx, step="quantile")
    d = _DATA[idx]
    m, om = _modules(c, d, dev)
    om.act_numel = d["x"].size
    return c, d, m, om


def _sets(c, slabs, seed):
    """S1 by rule from the plan's slab count, S2 seeded off it"""
    stages, nstage = batch_plan(c, slabs)
    full = stages // nstage  # chunks of nstage whole stages
    # (the middle chunk an odd one: with an odd nstage and two stages an image, N2, those start mid-image)
    chunks = [0, min(full // 2 | 1, full - 1), full - 1] + ([slabs - 1] if slabs > full else [])
    s1 = sorted({b for k in chunks for b in stage_images(c, nstage, k)} | {0, c["B"] - 1})
    for k in chunks[:3]:
        # every stage position of the chunk: its images' pixels cover the chunk's nstage stages
        P = c["H"] * c["W"]
        held = {s for b in stage_images(c, nstage, k) for s in range(b * P // 128, -(-(b + 1) * P // 128))}
        assert set(range(k * nstage, (k + 1) * nstage)) <= held
    assert len(s1) <= 16
    rest = np.setdiff1d(np.arange(c["B"]), s1)
    s2 = sorted(np.random.default_rng(seed).choice(rest, N_RANDOM, replace=False).tolist())
    return s1, s2


def _masked(g, sel):
    out = np.zeros_like(g)
    out[sel] = g[sel]
    return out


def _oracle(c, d, om, box, sel):
    """the module oracle on x[sel], g[sel] with the whole batch's step sizes: every reference and its term sums"""
    x, w, g = d["x"][sel], d["w"], d["g"][sel]
    for n in PARAMS:
        getattr(om, n).grad = None
    ox = torch.from_numpy(x).requires_grad_(True)
    oout = om(ox)
    cc, dd = box["c"], om.dbg
    # grad_alpha_cim's factor 1 / sqrt(ps.numel() * Qp_adc) (lsq.py:323) counts the whole batch's partial sums
    cc.meta["ps_numel"] = cc.ps16.size // len(sel) * d["x"].shape[0]
    oout.backward(torch.from_numpy(g))
    bm = om.binary_mask.numpy()
    terms = (np.abs(cc.adc.astype(np.float64)) * np.abs(bm.astype(np.float64))).sum(axis=(1, 2, 3))
    n, O = g.shape[:2]
    ax, aw, aa = co.cim_backward(cc, np.ascontiguousarray(g.reshape(n, O, -1).transpose(0, 2, 1)), absolute=True)
    np_ = lambda t: t.detach().numpy()  # noqa: E731
    return dict(
        dd=dd, out=np_(oout), out_terms=terms.transpose(0, 2, 1).reshape(oout.shape),
        gx=np_(ox.grad), ax=ax.reshape(x.shape), gw=np_(om.weight.grad), aw=aw.reshape(w.shape),
        ga=np_(om.alpha_cim.grad), aa=aa, g_act=om.alpha_act.grad.item(), g_w=om.alpha_weight.grad.item(),
        # (grad_scale's factors are the whole batch's, as in the oracle's forward)
        t_act=_lsq_scalar_terms(x, dd["x_q"].grad.numpy(), dd["sa"].item(), 0, d["qp_a"],
                                1.0 / math.sqrt(d["x"].size * d["qp_a"])),
        t_w=_lsq_scalar_terms(w, dd["w_q"].grad.numpy(), dd["sw"].item(), d["qn_w"], d["qp_w"],
                              1.0 / math.sqrt(w.size * d["qp_w"])))


def _against_oracle(tag, o, sel, a_cim, out, gx, pg):
    """a masked run's outputs against the oracle of its set; the figures, printed before they are asserted"""
    np_ = lambda t: t.detach().cpu().numpy()  # noqa: E731
    errs = dict(out=rel_err(np_(out)[sel], o["out"], o["out_terms"]), grad_x=rel_err(np_(gx)[sel], o["gx"], o["ax"]),
                grad_w=rel_err(np_(pg[0]), o["gw"], o["aw"]))
    ga, gr = np_(pg[3]), o["ga"]
    inner = (a_cim != a_cim.max()) & (a_cim != a_cim.min())
    errs["grad_alpha_cim"] = rel_err(ga[inner], gr[inner], np.broadcast_to(o["aa"], gr.shape)[inner])
    edge = np.abs(ga - gr).max() / np.abs(gr).max()
    e_act, e_w = abs(pg[1].item() - o["g_act"]) / o["t_act"], abs(pg[2].item() - o["g_w"]) / o["t_w"]
    outside = np.setdiff1d(np.arange(gx.shape[0]), sel)
    stray = float(gx[torch.from_numpy(outside).to(gx.device)].abs().max())
    print(f"{tag}: {errs}, grad_alpha_cim max/min entries {edge:.3e}, alpha_act {e_act:.3e}, alpha_weight {e_w:.3e} "
          f"of their term sums, largest |grad_x| off the set {stray}")
    assert all(e < 1e-5 for e in errs.values()), (tag, errs)
    assert edge <= 1e-5, (tag, "grad_alpha_cim (max / min entries)", edge)
    assert e_act <= 1e-5 and e_w <= 1e-5, (tag, e_act, e_w)
    assert stray == 0.0, (tag, "grad_x of an image whose grad_out is zero", stray)


@pytest.mark.parametrize("idx", range(len(BATCH_CASES)), ids=[case_id(c) for c in BATCH_CASES])
def test_backward_vs_sampled_oracle(cuda_device, monkeypatch, idx):
    import cim_quantization_amd._lib as L
    from cim_quantization_amd import functional as F
    c, d, m, om = _case(idx, cuda_device)
    x, w, g = d["x"], d["w"], d["g"]
    desc = F.module_descs(m, tuple(x.shape))[0]
    ok, chunks, bands, slabs = L.module_wide_bwd_plan(desc)
    stages, nstage = batch_plan(c, max(slabs, 1))
    print(f"{case_id(c)}: (ok, chunks, bands, slabs) = {(ok, chunks, bands, slabs)}, ceil(H / bands) = "
          f"{-(-c['H'] // max(bands, 1))}, {stages} stages, nstage = {nstage}")
    assert ok == 1 and (bands, slabs) == c["plan"] and -(-c["H"] // bands) > 1 and nstage > 1
    s1, s2 = _sets(c, slabs, 9970 + idx)
    print(f"{case_id(c)}: S1 = {s1}, S2 = {s2}")

    # the stateless forward, then the dense run twice
    m.wide_backward = False
    with torch.no_grad():
        out0 = m(torch.from_numpy(x).to(cuda_device))
    assert _routes(m, x.shape) == WIDE
    out, gx, pg = _run(m, x, g, cuda_device, True)
    assert _routes(m, x.shape) == WIDE_BWD
    assert torch.equal(out, out0)  # the state instances add in the stateless instances' order
    out2, gx2, pg2 = _run(m, x, g, cuda_device, True)
    assert torch.equal(out2, out) and torch.equal(gx2, gx)
    assert all(torch.equal(a, b) for a, b in zip(pg2, pg))

    # the oracles, on the module's own step sizes bit for bit
    box = _capture_oracle_ctx(monkeypatch)
    o1 = _oracle(c, d, om, box, s1)
    dd = o1["dd"]
    for mine, ref, n, qp in ((m.alpha_act, dd["sa"], x.size, d["qp_a"]), (m.alpha_weight, dd["sw"], w.size, d["qp_w"])):
        step = F.act_code_step(mine, 1.0 / math.sqrt(n * qp)).cpu()
        assert torch.equal(step.view(torch.int32), ref.detach().reshape(1).view(torch.int32))
    alpha_q = co.alpha_quantize(om.alpha_cim.detach().numpy(), 8)
    oc, _ = _oracle_codes(dd["x_q"].detach().numpy(), dd["w_q"].detach().numpy(), c["s"], c["p"], c["wb"], c["xbar"],
                          alpha_q, dd["sw"].detach().numpy().reshape(1), dd["sa"].detach().numpy().reshape(1), 0.0,
                          ab=c["ab"], wbs=c["wbs"], abs_=c["abs"])
    _coverage(c, dd, d, oc)
    o2 = _oracle(c, d, om, box, s2)
    a_cim = om.alpha_cim.detach().numpy()

    # one masked run per set
    r1 = _run(m, x, _masked(g, s1), cuda_device, True)
    assert torch.equal(r1[0], out)
    _against_oracle(case_id(c) + " S1", o1, s1, a_cim, *r1)
    r2 = _run(m, x, _masked(g, s2), cuda_device, True)
    _against_oracle(case_id(c) + " S2", o2, s2, a_cim, *r2)

    # the dense run's grad_x on both sets (grad_x is per image)
    for tag, sel, o in (("S1", s1, o1), ("S2", s2, o2)):
        e = rel_err(gx.cpu().numpy()[sel], o["gx"], o["ax"])
        print(f"{case_id(c)} dense grad_x[{tag}]: {e:.3e}")
        assert e < 1e-5, (tag, e)

    # additivity over S1 / its complement
    rest = np.setdiff1d(np.arange(c["B"]), s1)
    rc = _run(m, x, _masked(g, rest), cuda_device, True)
    for n, a, b, full in zip(PARAMS, r1[2], rc[2], pg):
        e = float(((a + b) - full).abs().max() / full.abs().max())
        print(f"{case_id(c)} additivity, grad of {n}: {e:.3e}")
        assert e <= 1e-5, (n, e)
