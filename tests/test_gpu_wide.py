"""GPU: module layers on the channel-chunked forward, cim_fwd_wide_kernel (wide_cases.py, B = 2).

Every case asserts its route -- (wide, general, general), forward only (wide, none, none) -- and its plan before it
launches: on a library without the route the case stops there.

Bars.  The training forward's out against the module oracle on the whole batch: 1e-5 of max(|ref|, sum of |terms|)
(conftest.rel_err, the helper of the w4a4 tests), and the general backward behind it on W1 and W5 at the same bar.
Every forward-only mode against the training forward of the same layer on the same parameters: torch.equal (bit
patterns where NaNs may occur) -- the training call quantises x in prep_module_kernel, the forward-only call in the
kernel's row staging.  forward_fused against the four torch operations on forward's output: torch.equal.
The coverage conditions are asserted on the oracle's values (5-95 % nonzero codes in every slice pair, >= 1 % of the
activations at Qp, weights at both clamp ends).
"""
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err
from oracle import cim_oracle as co
from rect_cases import make_desc, out_hw, route_names
from test_gpu_epilogue import _fused, _plain, _ref, _tables
from test_gpu_fullsize import _capture_oracle_ctx, _lsq_scalar_terms, _oracle_codes
from test_gpu_rect import _module_data, _modules
from wide_cases import BACKWARD, CASES, FUSED, TERNARY, W1, W3, W4, WIDE, case_id

pytestmark = pytest.mark.gpu


def _F():
    from cim_quantization_amd import functional as F
    return F


def _L():
    import cim_quantization_amd._lib as L
    return L


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_wide(c, m, x_shape):
    """the route and plan of the table's descriptor and of the descriptors the module itself makes for this input"""
    F, L = _F(), _L()
    assert L.load().cimq_wide_abi() == 1
    assert c["route"] == WIDE and route_names(L, make_desc(L, c)) == WIDE
    d = F.module_descs(m, tuple(x_shape))[0]
    assert route_names(L, d) == WIDE
    di = F.module_descs(m, tuple(x_shape), inference=True)[0]
    assert route_names(L, di) == ("wide", "none", "none") and L.module_forward_form(di)[1] == 1
    plan = L.module_wide_plan(d)
    assert plan[0] == 1 and plan[3] == -(-c["C"] * c["kh"] * c["kw"] // c["xbar"])
    return plan


_DATA = {}


def _two_bit_weight_step(c, d, seed, q=0.6):
    """2-bit weights hold -2 .. 1 and their top slice is set for -2 alone: at the 97 % point of |w| that code is 0.05 %
    of the weights and the top slice's partial sums are 0 throughout.  The weight step at the 60 % point instead (a
    sixth of the weights at -2), and alpha_cim made from it as test_gpu_rect._module_data makes it."""
    rng = np.random.default_rng(seed)
    x, w = d["x"], d["w"]
    aw = np.float32(np.quantile(np.abs(w), q) / d["qp_w"])
    sa0 = co.grad_scale_value(np.array([d["aa"]], np.float32), 1.0 / math.sqrt(x.size * d["qp_a"]))
    sw0 = co.grad_scale_value(np.array([aw], np.float32), 1.0 / math.sqrt(w.size * d["qp_w"]))
    xq0, _ = co.lsq_quantize(x, sa0, 0, d["qp_a"])
    wq0, _ = co.lsq_quantize(w, sw0, d["qn_w"], d["qp_w"])
    ac = co.alpha_cim_init(xq0, wq0, c["s"], c["p"], c["ab"], c["abs"], c["wb"], c["wbs"], c["xbar"], sw0, sa0, c["adc"])
    ac = (ac * (0.7 + 0.6 * rng.random(ac.shape))).astype(np.float32)
    return dict(d, aw=aw, ac=ac)


def _case(idx, dev):
    """(case, data, module, oracle module) of case idx; the data and the oracle's outputs are made once"""
    c = CASES[idx]
    if idx not in _DATA:
        _DATA[idx] = _module_data(c, 9700 + idx, step="quantile")
        if c["wb"] == 2:
            _DATA[idx] = _two_bit_weight_step(c, _DATA[idx], 9800 + idx)
    d = _DATA[idx]
    m, om = _modules(c, d, dev)
    return c, d, m, om


def _train_out(m, x):
    m.train()
    return m(x.clone().requires_grad_(True)).detach()


def _unprepared(m, x):
    F = _F()
    with torch.no_grad():
        return F.cim_module_conv(x, m.weight, m.alpha_act, m.alpha_weight, m.alpha_cim, m.binary_mask.to(x.device),
                                 m.signed_act, *m.layer_config(), False, False, None, None, m.recompute_psum)


def _coverage(c, dd, d, oc=None):
    """on the oracle's values, every case: at least 1 % of the activations at Qp, weights at both clamp ends; with
    the ternary ADC's codes ``oc`` also 5-95 % nonzero codes in every slice pair"""
    xr = np.rint(dd["x_q"].detach().numpy() / dd["sa"].item())
    wr = np.rint(dd["w_q"].detach().numpy() / dd["sw"].item())
    at_qp = (np.abs(xr) == d["qp_a"]).mean()
    print(f"{case_id(c)}: activations at Qp {at_qp:.4f}, weights at Qn {(wr == d['qn_w']).mean():.4f}, at Qp "
          f"{(wr == d['qp_w']).mean():.4f}")
    assert at_qp >= 0.01
    assert (wr == d["qn_w"]).any() and (wr == d["qp_w"]).any()
    if oc is not None:
        nz = (oc != 0).mean(axis=(0, 1, 4, 5))  # per (k, j)
        print(f"{case_id(c)}: nonzero codes per slice pair {nz.min():.3f} .. {nz.max():.3f}")
        assert nz.min() >= 0.05 and nz.max() <= 0.95, nz


# ---------------------------------------------------------------------------------------------------
# 1. the training forward (and on W1 / W5 the general backward behind it) against the module oracle
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_training_forward_vs_oracle(cuda_device, monkeypatch, idx):
    c, d, m, om = _case(idx, cuda_device)
    x, w, g = d["x"], d["w"], d["g"]
    plan = _assert_wide(c, m, x.shape)
    if idx == W4:
        assert plan[1] >= 2  # several channel chunks
    if idx == W3:
        assert plan[2] >= 2  # several output groups
    ho, wo = out_hw(c)
    bwd = idx in BACKWARD
    xt = torch.from_numpy(x).to(cuda_device).requires_grad_(True)
    out = m(xt)
    assert tuple(out.shape) == (c["B"], c["O"], ho, wo) and out.is_contiguous()
    if bwd:
        out.backward(torch.from_numpy(g).to(cuda_device))
    torch.cuda.synchronize()

    box = _capture_oracle_ctx(monkeypatch)
    ox = torch.from_numpy(x).requires_grad_(True)
    oout = om(ox)
    cc = box["c"]
    bm = om.binary_mask.numpy()
    terms = (np.abs(cc.adc.astype(np.float64)) * np.abs(bm.astype(np.float64))).sum(axis=(1, 2, 3))
    terms = terms.transpose(0, 2, 1).reshape(oout.shape)
    e = rel_err(out.detach().cpu().numpy(), oout.detach().numpy(), terms)
    print(f"{case_id(c)}: out error {e:.3e} of max(|ref|, sum |terms|)")
    assert torch.isfinite(out).all() and float(out.detach().abs().max()) > 0
    assert e < 1e-5
    dd = om.dbg
    if idx not in TERNARY:
        _coverage(c, dd, d)
    if idx in TERNARY:
        alpha_q = co.alpha_quantize(om.alpha_cim.detach().numpy(), 8)
        oc, _ = _oracle_codes(dd["x_q"].detach().numpy(), dd["w_q"].detach().numpy(), c["s"], c["p"], c["wb"], c["xbar"],
                              alpha_q, dd["sw"].detach().numpy().reshape(1), dd["sa"].detach().numpy().reshape(1), 0.0,
                              ab=c["ab"], wbs=c["wbs"], abs_=c["abs"])
        _coverage(c, dd, d, oc)
    if bwd:
        oout.backward(torch.from_numpy(g))
        B, O = g.shape[:2]
        g_bpo = np.ascontiguousarray(g.reshape(B, O, -1).transpose(0, 2, 1))
        ax, aw, _ = co.cim_backward(cc, g_bpo, absolute=True)
        np_ = lambda t: t.detach().cpu().numpy()  # noqa: E731
        assert rel_err(np_(xt.grad), np_(ox.grad), ax.reshape(x.shape)) < 1e-5, "grad_x"
        assert rel_err(np_(m.weight.grad), np_(om.weight.grad), aw.reshape(w.shape)) < 1e-5, "grad_w"
        t_act = _lsq_scalar_terms(x, dd["x_q"].grad.numpy(), dd["sa"].item(), 0, d["qp_a"],
                                  1.0 / math.sqrt(x.size * d["qp_a"]))
        assert abs(m.alpha_act.grad.item() - om.alpha_act.grad.item()) <= 1e-5 * t_act
    # a second run: the same bits
    assert torch.equal(_train_out(m, torch.from_numpy(x).to(cuda_device)), out.detach())


# ---------------------------------------------------------------------------------------------------
# 2. forward only: prepared and unprepared, against the training forward; one launch per prepared layer
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_forward_only_equals_training_forward(cuda_device, idx):
    c, d, m, _ = _case(idx, cuda_device)
    x = torch.from_numpy(d["x"]).to(cuda_device)
    _assert_wide(c, m, x.shape)
    ref = _train_out(m, x)
    v = _plain(m, x)  # prepared: the kept inference weight side
    assert v.shape == ref.shape and v.is_contiguous()
    assert torch.equal(v, ref), float((v - ref).abs().max())
    u = _unprepared(m, x)
    assert torch.equal(_bits(u), _bits(v))
    assert torch.equal(_bits(_plain(m, x)), _bits(v))
    # the weight side is made once and kept while the layer evaluates (train() drops it)
    try:
        m.eval()
        with torch.no_grad():
            a = m(x)
            kept = m._inf_prep
            b = m(x)
        assert kept is not None and m._inf_prep is kept
        assert torch.equal(_bits(a), _bits(v)) and torch.equal(_bits(b), _bits(v))
    finally:
        m.train()


def _count_launches(fn):
    spec = importlib.util.spec_from_file_location("infer_net_bench", os.path.join(REPO, "tools", "infer_net_bench.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool.count_launches(fn)


def test_one_launch_per_prepared_layer(cuda_device):
    c, d, m, _ = _case(W1, cuda_device)
    x = torch.from_numpy(d["x"]).to(cuda_device)
    _assert_wide(c, m, x.shape)
    v = _plain(m, x)
    scale, shift, res = _tables(v, 31)
    try:
        m.eval()
        with torch.no_grad():
            m(x)  # makes the weight side; the counted calls find it
            n_plain = _count_launches(lambda: m(x))
            n_fused = _count_launches(lambda: m.forward_fused(x, scale, shift, residual=res, relu=True))
    finally:
        m.train()
    assert "error" not in n_plain and "error" not in n_fused, (n_plain, n_fused)
    print("device kernels: prepared forward %s, forward_fused %s" % (n_plain, n_fused))
    assert n_plain["kernels"] == n_plain["libcimq"] == 1
    assert n_fused["kernels"] == n_fused["libcimq"] == 1


def test_literal_flag(cuda_device):
    """W9: W1 with an all-equal alpha_cim -- the alpha quantiser's scale is 0, the literal ADC runs and the output is
    NaN throughout, in the training forward and in every forward-only call"""
    c, d, m, om = _case(W1, cuda_device)
    with torch.no_grad():
        m.alpha_cim.fill_(0.05)
        om.alpha_cim.fill_(0.05)
    x = torch.from_numpy(d["x"]).to(cuda_device)
    _assert_wide(c, m, x.shape)
    ref = _train_out(m, x)
    assert torch.isnan(ref).all()
    # the oracle on the same parameters: the same NaN pattern, on data that meets the coverage conditions
    om.train()
    oout = om(torch.from_numpy(d["x"]).requires_grad_(True)).detach()
    assert oout.shape == ref.shape and torch.equal(torch.isnan(oout), torch.isnan(ref.cpu()))
    _coverage(c, om.dbg, d)
    assert torch.equal(_bits(_plain(m, x)), _bits(ref))
    assert torch.equal(_bits(_unprepared(m, x)), _bits(ref))


def test_staging_edge_cases(cuda_device):
    """NaN, +-inf, negatives, .5 sa ties, values at and above Qp sa: the staged quantiser's words are the prologue's"""
    c, d, m, om = _case(W1, cuda_device)
    QP = d["qp_a"]
    om.train()
    om(torch.from_numpy(np.abs(d["x"])))
    sa = float(om.dbg["sa"].item())
    x = d["x"].copy()
    flat = x.reshape(-1)
    rng = np.random.default_rng(9771)
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
    _assert_wide(c, m, xt.shape)
    ref = _train_out(m, xt)
    assert float(ref.abs().nan_to_num().max()) > 0
    v = _plain(m, xt)
    assert torch.equal(_bits(v), _bits(ref)), float((v - ref).abs().nan_to_num().max())
    assert torch.equal(_bits(_unprepared(m, xt)), _bits(ref))


# ---------------------------------------------------------------------------------------------------
# 3. forward_fused: the epilogue instances
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", FUSED, ids=[case_id(CASES[i]) for i in FUSED])
def test_forward_fused(cuda_device, idx):
    c, d, m, _ = _case(idx, cuda_device)
    x = torch.from_numpy(d["x"]).to(cuda_device)
    _assert_wide(c, m, x.shape)
    assert m.fused_epilogue_ready(x) is True
    ref = _train_out(m, x)
    v = _plain(m, x)
    assert torch.equal(v, ref)
    scale, shift, res = _tables(v, 670 + idx)
    for kw in (dict(), dict(relu=True), dict(residual=res), dict(residual=res, relu=True)):
        got = _fused(m, x, scale, shift, **kw)
        want = _ref(ref, scale, shift, **kw)
        assert got.shape == v.shape and torch.equal(got, want), (kw.keys(), float((got - want).abs().max()))
    frac = float((_ref(ref, scale, shift, res, True) == 0).float().mean())
    assert 0.05 < frac < 0.95, frac  # (ReLU does cut, and not everything)
    a = _fused(m, x, scale, shift, residual=res, relu=True)
    assert torch.equal(a, _fused(m, x, scale, shift, residual=res, relu=True))


# ---------------------------------------------------------------------------------------------------
# 4. refusals: codes on either side leave the buffers untouched
# ---------------------------------------------------------------------------------------------------
def test_codes_are_refused(cuda_device):
    c, d, m, _ = _case(W1, cuda_device)
    x = torch.from_numpy(d["x"]).to(cuda_device)
    _assert_wide(c, m, x.shape)
    v = _plain(m, x)
    assert tuple(m.codes_ready(x)) == (False, False)
    scale, shift, _ = _tables(v, 77)
    xq = torch.zeros(x.shape, dtype=torch.uint8, device=cuda_device)
    with pytest.raises(Exception) as ei:
        _fused(m, xq, scale, shift)
    assert "wide route" in str(ei.value), str(ei.value)
    with pytest.raises(Exception) as ei:
        _fused(m, x, scale, shift, out_quant=m)
    assert "wide route" in str(ei.value), str(ei.value)
    torch.cuda.synchronize()
    assert torch.equal(_plain(m, x), v)  # the kept weight side is what it was


class _RawCodes:
    """cimq_module_forward_codes through ctypes on module m's parameters, every output buffer filled with a sentinel"""

    def __init__(self, m, x):
        from test_gpu_codes import _Raw
        self.r = _Raw(m, tuple(x.shape))
        self.r.oq.fill_(99)
        self.x = x

    def call(self, scale, shift, x_codes=None, out_codes=False):
        L, r = _L(), self.r
        p = lambda u: None if u is None else u.data_ptr()  # noqa: E731
        epi = L.make_epilogue(p(scale), p(shift), None, True)
        if out_codes:
            alpha, gs, qp = r.m._code_quant(r.out.numel())
            oa = alpha.detach().reshape(-1)[:1].contiguous()
            io = L.make_act_codes(p(x_codes), p(r.oq), p(oa), gs, qp, False)
        else:
            io = L.make_act_codes(x_codes=p(x_codes))
        rc = L.load().cimq_module_forward_codes(r.desc, r.lsq, ctypes.byref(io), None if x_codes is not None else p(self.x),
                                                *[p(u) for u in r.t], ctypes.byref(epi), p(r.out), p(r.cbuf), p(r.ws),
                                                torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc


def test_forward_codes_refused_buffers_untouched(cuda_device):
    """cimq_module_forward_codes with codes in, out or both on a wide layer: CIMQ_EUNSUPPORTED, out and out_codes as
    they were; without codes the same call runs"""
    L = _L()
    c, d, m, _ = _case(W1, cuda_device)
    x = torch.from_numpy(d["x"]).to(cuda_device)
    _assert_wide(c, m, x.shape)
    v = _plain(m, x)
    scale, shift, _ = _tables(v, 78)
    xq = torch.zeros(x.shape, dtype=torch.uint8, device=cuda_device)
    raw = _RawCodes(m, x)
    for kw in (dict(x_codes=xq), dict(out_codes=True), dict(x_codes=xq, out_codes=True)):
        assert raw.call(scale, shift, **kw) == L.CIMQ_EUNSUPPORTED, kw.keys()
        assert b"wide route" in L.load().cimq_last_error()
        assert bool((raw.r.out == 7.0).all()) and bool((raw.r.oq == 99).all())
    assert raw.call(scale, shift) == 0, L.load().cimq_last_error()
    assert torch.equal(raw.r.out, _ref(v, scale, shift, relu=True)) and bool((raw.r.oq == 99).all())


def test_net_refusals_buffers_untouched(cuda_device):
    """a cimq_net_forward plan whose wide layer has codes or a residual view: CIMQ_EUNSUPPORTED before any launch, no
    slot touched; the same layers with fp32 edges and a whole-tensor residual run, equal to the loop"""
    from test_gpu_net import _Plan, _mk
    L = _L()
    c, d, m, _ = _case(W1, cuda_device)
    x = torch.from_numpy(d["x"]).to(cuda_device)
    _assert_wide(c, m, x.shape)
    v = _plain(m, x)
    s1, t1, _ = _tables(v, 79)
    y1 = _fused(m, x, s1, t1, relu=True)
    m2 = _mk(cuda_device, 128, 128, 1, y1, 9781)   # a second wide layer, reading the first one's output
    half = _mk(cuda_device, 128, 64, 1, x, 9782)   # 64 channels: the source of a residual view
    _assert_wide(c, m2, y1.shape)
    s2, t2, _ = _tables(_plain(m2, y1), 80)
    sh, th, _ = _tables(_plain(half, x), 81)
    want = _fused(m2, y1, s2, t2, residual=y1, relu=True)
    try:
        for mod in (m, m2, half):
            mod.eval()
        # codes between the two wide layers
        p = _Plan(x)
        a, b = p.slot(y1.shape, codes=True), p.slot(want.shape)
        p.layer(m, x.shape, s1, t1, True, -1, a, out_mode=3, consumer=1)
        p.layer(m2, y1.shape, s2, t2, True, a, b, in_codes=1)
        assert p.run(expect=L.CIMQ_EUNSUPPORTED) == L.CIMQ_EUNSUPPORTED
        assert b"wide route" in L.load().cimq_last_error()
        assert bool((p.sf[a] == 7.0).all()) and bool((p.sc[a] == 99).all()) and bool((p.sf[b] == 7.0).all())
        # a residual view: 64 source channels from channel 32 into the 128 of a wide layer that reads x itself
        p = _Plan(x)
        a, b = p.slot(_plain(half, x).shape), p.slot(v.shape)
        p.layer(half, x.shape, sh, th, True, -1, a)
        p.layer(m, x.shape, s1, t1, True, -1, b, res_slot=a, res_c0=32)
        assert p.run(expect=L.CIMQ_EUNSUPPORTED) == L.CIMQ_EUNSUPPORTED
        assert b"wide route reads no residual view" in L.load().cimq_last_error()
        assert bool((p.sf[a] == 7.0).all()) and bool((p.sf[b] == 7.0).all())
        # fp32 edges and the whole tensor as the residual: the plan runs
        p = _Plan(x)
        a, b = p.slot(y1.shape), p.slot(want.shape)
        p.layer(m, x.shape, s1, t1, True, -1, a)
        p.layer(m2, y1.shape, s2, t2, True, a, b, res_slot=a)
        p.run()
    finally:
        for mod in (m, m2, half):
            mod.train()
    assert torch.equal(_bits(p.sf[a]), _bits(y1)) and torch.equal(_bits(p.sf[b]), _bits(want))


# ---------------------------------------------------------------------------------------------------
# 5. VGG-small: FusedEval and the launcher
# ---------------------------------------------------------------------------------------------------
def _vgg(dev):
    """cifar10_vggsmall with every conv a Conv2dLSQCiM (w3a3, the first w8a8) after one training step at B = 2 (the
    first-step initialisations), its BatchNorms given random statistics, in evaluation mode"""
    import cim_quantization_amd._modules as my_nn
    from cim_quantization_amd.harness import models
    from cim_quantization_amd.harness.replace import ReplaceModuleTool
    from test_epilogue_host import randomise_bn
    torch.manual_seed(31)
    model = models.cifar10_vggsmall()
    ReplaceModuleTool(model, {"Conv2d": [my_nn.Conv2dLSQCiM]}, True, nbits_w=3, nbits_a=3, nbits_alpha=8, wbitslice=1,
                      abitslice=1, xbar=128, adcbits=1.5, signed_xbar=True, stochastic_quant=False).replace()
    model = model.to(dev).train()
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(32)).to(dev)
    model(x)
    randomise_bn(model, 33)
    return model.eval(), x


def test_fused_eval_vgg(cuda_device):
    import cim_quantization_amd._modules as my_nn
    from cim_quantization_amd.harness.fuse import FusedEval, fold_bn
    F, L = _F(), _L()
    model, x = _vgg(cuda_device)
    mods = list(model.features)
    convs = [m for m in mods if isinstance(m, my_nn.Conv2dLSQCiM)]
    assert len(convs) == 6 and convs[0].nbits_w == 8
    with torch.no_grad():
        # the same loop with conv(x) and the four torch operations
        y, routes, i = x, [], 0
        while i < len(mods):
            if isinstance(mods[i], my_nn.Conv2dLSQCiM):
                d = F.module_descs(mods[i], tuple(y.shape), inference=True)[0]
                routes.append(L.ROUTE_NAMES[L.module_route(d)[0]])
                scale, shift = fold_bn(mods[i + 1])
                v = mods[i](y) * scale.view(1, -1, 1, 1)
                y = torch.relu(v + shift.view(1, -1, 1, 1))
                i += 3
            else:
                y = mods[i](y)
                i += 1
        want = model.classifier(y.flatten(1))
        assert routes == ["v3"] + ["wide"] * 5
        fused = FusedEval(model)
        got = fused(x)
        assert torch.isfinite(got).all() and torch.equal(got, want), float((got - want).abs().max())
        assert torch.equal(fused(x), got)
        fc = FusedEval(model, codes=True)
        assert torch.equal(fc(x), got) and fc.code_edges == []
        fn = FusedEval(model, net=True)
        assert torch.equal(fn(x), got)
        assert fn.net_used is False and fn.net_reason


def test_fused_eval_narrow_vgg_hands_codes(cuda_device):
    """a VGG of 16 / 32 / 64 channels: with codes=True the conv -> conv edges carry codes (codes_ready holds on both
    sides), the edges into the max-pools stay fp32, and the logits are FusedEval(model)'s bit for bit"""
    import cim_quantization_amd._modules as my_nn
    from cim_quantization_amd.harness import models
    from cim_quantization_amd.harness.fuse import FusedEval
    from cim_quantization_amd.harness.replace import ReplaceModuleTool
    from test_epilogue_host import randomise_bn
    torch.manual_seed(41)
    model = models.VGG(plan=(16, 16, "M", 32, 32, "M", 64, 64, "M"))
    ReplaceModuleTool(model, {"Conv2d": [my_nn.Conv2dLSQCiM]}, True, nbits_w=3, nbits_a=3, nbits_alpha=8, wbitslice=1,
                      abitslice=1, xbar=128, adcbits=1.5, signed_xbar=True, stochastic_quant=False).replace()
    model = model.to(cuda_device).train()
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(42)).to(cuda_device)
    model(x)
    randomise_bn(model, 43)
    model.eval()
    with torch.no_grad():
        want = FusedEval(model)(x)
        fc = FusedEval(model, codes=True)
        got = fc(x)
    assert torch.isfinite(want).all() and torch.equal(got, want)
    assert fc.code_edges == [("features.0", "features.3", "codes"), ("features.7", "features.10", "codes"),
                             ("features.14", "features.17", "codes")]


VGG_PROTO = """
arch: "cifar10_vggsmall"
model_source: Local
log_name: "{log}"
data: "{data}"
lr: 0.01
epochs: 1
batch_size: 8
print_freq: 1
seed: 0
gpu_id: ANY
nbits_w: 3
nbits_a: 3
nbits_alpha: 8
wbitslice: 1
abitslice: 1
xbar: 128
adcbits: 1.5
lr_scheduler: CosineAnnealingLR
optimizer: SGD
sgd {{ weight_decay: 1e-4 momentum: 0.9 }}
{extra}
"""


def test_harness_trains_vggsmall(cuda_device, tmp_path, capsys):
    """train -> checkpoint -> resume -> evaluate (also through FusedEval) on a cifar10_vggsmall prototxt, two steps"""
    from cim_quantization_amd._modules.lsq import Conv2dLSQCiM
    from cim_quantization_amd.harness import train
    from test_gpu_harness import _data
    _data(str(tmp_path))
    log = str(tmp_path / "run")
    hp1 = tmp_path / "train.prototxt"
    hp1.write_text(VGG_PROTO.format(log=log, data=str(tmp_path), extra=""))
    best = train.main(["--hp", str(hp1), "--max-steps", "2", "--max-val-steps", "1"])
    out = capsys.readouterr().out
    assert np.isfinite(best)
    losses = [float(ln.split("loss ")[1].split()[0]) for ln in out.splitlines() if ln.startswith("Epoch [")]
    assert len(losses) == 2 and all(np.isfinite(losses))
    ck_path = os.path.join(log, "cifar10_vggsmall_Conv2dLSQCiMcheckpoint.pth.tar")
    ck = torch.load(ck_path, map_location="cpu", weights_only=True)
    assert ck["arch"] == "cifar10_vggsmall_Conv2dLSQCiM" and "optimizer" in ck
    sd = ck["state_dict"]
    assert sd["features.3.alpha_cim"].shape == (1, 9, 3, 3, 1, 128) and float(sd["features.3.init_state"]) == 1.0
    assert sd["classifier.weight"].shape == (10, 8192)
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
    hp2 = tmp_path / "eval.prototxt"
    hp2.write_text(VGG_PROTO.format(log=log, data=str(tmp_path), extra=f'evaluate: true\nresume: "{ck_path}"'))
    acc = train.main(["--hp", str(hp2), "--max-val-steps", "1"])
    acc_f = train.main(["--hp", str(hp2), "--max-val-steps", "1", "--fused-eval"])
    model, _ = train.build_model(train.load_hyperparam(str(hp2)), cuda_device)
    assert isinstance(model.features[17], Conv2dLSQCiM)
    assert torch.equal(model.features[17].alpha_cim.detach().cpu(), sd["features.17.alpha_cim"])
    assert np.isfinite(acc) and np.isfinite(acc_f)
